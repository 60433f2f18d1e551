"""A float64 reference on SAMPLED ROWS of a large batch (test infrastructure; imported by tests/test_hip_rows_f64.py and
tests/test_rows_f64_cpu.py -- a plain module, not a conftest).

Rays are independent: the outputs of a set R of rows depend on those rows' inputs alone, and so does the exact parameter gradient of
sum(C * out) when the cotangent C is zero outside R.  So the oracle (oracle/vipnerf_oracle.py), run in float64 on R's rows with the same
float32 inputs upcast exactly and HIP's own coarse / fine depths teacher-forced, checks a HIP call of any size -- 10 000+ rays, where the
float32 oracle with autograd (~700 rays/s) cannot follow.  A one-ray cotangent turns a lost block of points into a 100 % error.

The second half mirrors the weight-gradient point-chunk planner of the library, so that R can hold the rays whose points straddle a chunk
boundary: vipnerf_common.h (wgrad_chunks, wgrad_chunk_pts, wgrad_chunks_split, wgrad_partial_total, bwd_layout), the fp32 / fp16x3 plan of
vipnerf_wgrad.hip (launch_wgrad: the 256 x 256 class keeps wgrad_chunks / wgrad_chunk_pts) and the per-class plan of vipnerf_wgrad16.hip
(launch_wgrad16: fp16x3h, fp16, bf16).  tests/test_rows_f64_cpu.py pins the mirror against vipnerf_query_workspace."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import vipnerf_oracle as vo  # noqa: E402

# ------------------------------------------------------------------------------------------------ the planner, mirrored
WGRAD_CHUNK_PTS = 8192          # vipnerf_common.h:89-90
WGRAD_MAX_CHUNKS = 256
WGRAD_SPLIT_PE, WGRAD_SPLIT_THIN, WGRAD_SINGLE_SPLIT = 8, 16, 8     # vipnerf_common.h:106
WG16_BIG_SLOTS = 256            # vipnerf_knobs.h VN_WG16_BIG_SLOTS
T16 = ('fp16x3h', 'fp16', 'bf16')     # stores_t16 (vipnerf_bf16n.h): their weight gradients run launch_wgrad16


def wgrad_chunks(P):
    """vipnerf_common.h:95-101"""
    rnd = 32 * WGRAD_CHUNK_PTS
    c = 32 * ((P + rnd - 1) // rnd)
    c = min(c, (P + 1023) // 1024)
    return max(1, min(c, WGRAD_MAX_CHUNKS))


def wgrad_chunk_pts(P):
    """vipnerf_common.h:108-112: ceil(P / n) rounded UP to 512 -- n is not re-derived, so the last chunks can start past P (empty)"""
    n = wgrad_chunks(P)
    c, q = (P + n - 1) // n, 32 * WGRAD_SPLIT_THIN
    return q if c == 0 else (c + q - 1) // q * q


def wgrad_chunks_split(P, split):
    """vipnerf_common.h:113-116"""
    c = wgrad_chunk_pts(P) // split
    return (P + c - 1) // c


def wgrad_partial_total(P, V):
    """vipnerf_common.h:118-125 (floats)"""
    big = 8 * (256 * 256 + 256) + 320
    pe = 2 * (256 * 64 + 256)
    single = (32 * 256 + 32) + (128 * 256 + 128)
    thin = (1 + V) * (128 * 32 + 128) + (1 + V) * (32 * 128 + 32)
    return (wgrad_chunks(P) * big + wgrad_chunks_split(P, WGRAD_SPLIT_PE) * pe + wgrad_chunks_split(P, WGRAD_SINGLE_SPLIT) * single
            + wgrad_chunks_split(P, WGRAD_SPLIT_THIN) * thin)


def bwd_layout_total(P, V, max_sec=3):
    """floats of vipnerf_common.h:126-145 bwd_layout(P, V) for fp32 storage (h16 = t16 = false; VIPNERF_MAX_SEC = 3)"""
    o = 8 * P * 256 + P * 256                      # dy[0..7], dyf
    o += (V + 1) * P * 128 + P * 128               # dyv per direction, dyvsum
    o += (V + 1) * P * 8                           # dq per direction
    o += P + 3 * P + P + P * max(V, 1)             # dsig, drgb, dvis, dvis2
    o = (o + 63) & ~63
    o += 64                                        # gmax
    return o + wgrad_partial_total(P, V)


def _wg16_plan(P, n_old, pts_old, slots, n_desc):
    """vipnerf_wgrad16.hip:498-503 (plan): one round of workgroups of the class where the level is large enough"""
    target = slots // n_desc
    if target >= n_old:
        return n_old, pts_old
    pts = ((P + target - 1) // target + 31) // 32 * 32
    return (P + pts - 1) // pts, pts


def big_class_plan(P, prec):
    """(chunks, points per chunk) of the 256 x 256 weight-gradient class (eight GEMMs of a level) in precision `prec`"""
    if prec in T16:
        return _wg16_plan(P, wgrad_chunks(P), wgrad_chunk_pts(P), WG16_BIG_SLOTS, 8)     # vipnerf_wgrad16.hip:506
    return wgrad_chunks(P), wgrad_chunk_pts(P)                                          # vipnerf_wgrad.hip:1469-1470


def empty_chunks(P, prec):
    """chunks of the 256 x 256 class that start at or past P (their workgroups must write a zero partial)"""
    n, pts = big_class_plan(P, prec)
    return n - min(n, -(-P // pts))


def boundary_rays(n_rays, S, prec):
    """rays whose S points straddle an inner chunk boundary of the 256 x 256 class (points p of ray r: r S .. r S + S - 1)"""
    P = n_rays * S
    n, pts = big_class_plan(P, prec)
    out = []
    for k in range(1, n):
        b = k * pts
        if b >= P:
            break
        r = b // S
        if b % S:                     # the boundary falls inside ray r
            out.append(r)
    return out


# ------------------------------------------------------------------------------------------------ the float64 reference
LEVEL_KEYS = ('rgb', 'acc', 'alpha', 'visibility', 'weights', 'depth', 'depth_var', 'depth_ndc', 'depth_var_ndc', 'visibility2',
              'raw_sigma', 'raw_rgb', 'raw_visibility', 'raw_visibility2')


def diff_keys(out):
    """the differentiable output keys of both levels present in a HIP module output (raw_rgb_view_dependent_* is an alias of raw_rgb_*)"""
    return [f'{k}_{lv}' for lv in ('coarse', 'fine') for k in LEVEL_KEYS if f'{k}_{lv}' in out]


def rows_batch(b, rows, dtype=torch.float64):
    """R's rows of a synthetic batch, floating tensors upcast exactly (masks, pixel ids kept; poses whole)"""
    idx = torch.as_tensor(rows, dtype=torch.long)
    n = b['rays_o'].shape[0]
    sub = {}
    for k, v in b.items():
        if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == n and k != 'poses':
            v = v[idx]
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            v = v.to(dtype)
        sub[k] = v
    return sub


def reference_rows(params, b, rng, rows, z_coarse, z_fine, cfg_o, sec_views=True):
    """float64 outputs of R's rows.  rng: the injected float32 numbers of the whole batch; z_coarse / z_fine: HIP's depths of R's rows
    (teacher forcing: the importance sampler is ill-conditioned).  -> (float64 parameters with requires_grad, outputs).

    The sample positions o + z d are formed in float32, as every float32 pipeline forms them, and upcast (oracle cfg `points_f32`): the
    positional encoding's top frequency, sin(2^9 x), turns their float32 rounding into ~1e-3 of the first layer's gradient -- measured
    between the float32 oracle itself and a float64 evaluation at exact positions (3e-3 .. 6e-3 rel. L2 per key on 64 fern rows; 1e-6 at
    the float32-formed positions).  The positions are an input of the network, not a computation the kernels can do better."""
    idx = torch.as_tensor(rows, dtype=torch.long)
    p = vo.params_to_torch(params, requires_grad=True, dtype=torch.float64)
    r = {k: v[idx].double() for k, v in rng.items() if isinstance(v, torch.Tensor)}
    r['z_coarse'] = z_coarse.double()
    r['z_fine'] = z_fine.double()
    out = vo.render_rays(p, rows_batch(b, rows), dict(cfg_o, points_f32=True), r, train=True, sec_views=sec_views)
    return p, out


def cotangents(ref, keys, shapes, rows, n_rays, seed):
    """A seeded cotangent on every key, non-zero on R's rows only, each key scaled by 1 / max |ref| (as test_depth_var_cotangents_vs_oracle).
    shapes: the HIP tensors' shapes.  -> {key: float32 (n_rays, ...)}; the float64 side uses the same values on R's rows."""
    gen = torch.Generator().manual_seed(seed)
    idx = torch.as_tensor(rows, dtype=torch.long)
    cts = {}
    for k in keys:
        shp = tuple(shapes[k])
        scale = max(float(ref[k].detach().abs().max()), 1e-6)
        full = torch.zeros(shp, dtype=torch.float32)
        full[idx] = (torch.randn((len(rows),) + shp[1:], generator=gen) / scale).float()
        cts[k] = full
    return cts


def reference_grads(p, ref, cts, rows, names, retain=False):
    """float64 gradient of sum(C * out) over R's rows, for every parameter in `names`"""
    idx = torch.as_tensor(rows, dtype=torch.long)
    tot = 0
    for k, c in cts.items():
        cr = c[idx].double()
        tot = tot + (ref[k].reshape(cr.shape) * cr).sum()
    g = torch.autograd.grad(tot, [p[k] for k in names], allow_unused=True, retain_graph=retain)
    return {k: (torch.zeros_like(p[k]) if gi is None else gi).detach() for k, gi in zip(names, g)}


def single_row(cts, r):
    """the cotangents restricted to row r"""
    out = {}
    for k, c in cts.items():
        z = torch.zeros_like(c)
        z[r] = c[r]
        out[k] = z
    return out


# ------------------------------------------------------------------------------------------------ bounds
# About twice what the first MI355X pass measured (profiles/r07_rows_f64_measured.txt: 14 cases, 82 rows each), per arithmetic class:
#   out        max |hip - ref| / max |ref| over R's rows, per output key (measured fp32 / fp16x3 / fp16x3h 7.7e-7, fp16 8.8e-5, bf16 9.5e-4)
#   depth_eps  the per-weight error of the depth statistics' per-ray first-order bound (tests/test_hip_rows_f64.py::depth_ratio; measured
#              at most 0.21 of it)
#   grad       rel. L2 per parameter tensor of the R-row backward; the element bound is 10 x.  Measured fp32 3.1e-4 .. 2.8e-3, fp16x3 /
#              fp16x3h 6.7e-4 .. 1.9e-3, fp16 5.7e-2, bf16 0.42: at fp32 grade these are KINK events -- every tensor of a level off by about
#              the same amount, one ray of R whose ReLU pre-activation sits at rounding level (one-ray backwards of the same inputs: 7e-7)
#   one_kink   rel. L2 of every tensor of EVERY one-ray backward (a ray with a kink: measured fp32 2.7e-2, fp16x3 1.2e-2, fp16x3h 6.8e-3, fp16
#              6.6e-2, bf16 0.21) -- a lost ray is 1, a lost 32-point block ~0.2 .. 0.5
#   one_median the median over a case's one-ray backwards of their worst tensor (measured fp32 9.9e-7, fp16x3 4.1e-6, fp16x3h 6.3e-4, fp16
#              5.7e-2, bf16 0.15): what a systematic error of 1e-3 cannot pass at fp32 grade
BOUNDS = {
    'fp32':    {'out': 2e-6, 'depth_eps': 1e-4, 'grad': 6e-3, 'one_kink': 6e-2, 'one_median': 2e-6},
    'fp16x3':  {'out': 2e-6, 'depth_eps': 1e-4, 'grad': 4e-3, 'one_kink': 3e-2, 'one_median': 1e-5},
    'fp16x3h': {'out': 2e-6, 'depth_eps': 1e-4, 'grad': 4e-3, 'one_kink': 1.5e-2, 'one_median': 1.3e-3},
    'fp16':    {'out': 2e-4, 'depth_eps': 5e-3, 'grad': 1.2e-1, 'one_kink': 1.4e-1, 'one_median': 1.2e-1},
    'bf16':    {'out': 2e-3, 'depth_eps': 4e-2, 'grad': 8.5e-1, 'one_kink': 4.5e-1, 'one_median': 3.5e-1},
}


def output_error(h, r):
    """max |h - r| / max |r| of one key (float64)"""
    h, r = h.detach().cpu().double().reshape(r.shape), r.detach().double()
    assert torch.isfinite(h).all()
    return float((h - r).abs().max() / r.abs().max().clamp_min(1e-30))


def grad_error(a, ref):
    """(rel. L2, largest element error / largest element) of one parameter tensor against its float64 gradient"""
    a, ref = np.asarray(a, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert np.isfinite(a).all()
    nrm = max(np.linalg.norm(ref), 1e-300)
    return float(np.linalg.norm(a - ref) / nrm), float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def check_grads(got, ref, bound, what):
    """every parameter's gradient against float64: rel. L2 <= bound and largest element error <= 10 x bound; a parameter the cotangent
    reaches (non-zero float64 gradient) must have a non-zero gradient.  -> worst rel. L2"""
    worst = 0.0
    for k, r in ref.items():
        r = r.detach().cpu().double().numpy() if isinstance(r, torch.Tensor) else np.asarray(r, np.float64)
        a = got[k].detach().cpu().double().numpy() if isinstance(got[k], torch.Tensor) else np.asarray(got[k], np.float64)
        if not np.abs(r).max() > 0:
            assert not np.abs(a).max() > 0, f'{what}: {k} must have no gradient'
            continue
        assert np.abs(a).max() > 0, f'{what}: {k} gets no gradient'
        l2, mx = grad_error(a, r)
        assert l2 <= bound and mx <= 10 * bound, f'{what}: {k} rel L2 {l2:.3e} (bound {bound:.1e}), max err / max|g| {mx:.3e}'
        worst = max(worst, l2)
    return worst


def check_one_rays(pairs, bd, what):
    """one-ray backwards [(ray, hip grads, float64 grads)]: every one reaches every parameter its float64 gradient does and stays within the
    kink bound; the median of their worst tensors within the fp32-grade bound.  -> (median, worst)"""
    worst = []
    for r, got, ref in pairs:
        worst.append(check_grads(got, ref, bd['one_kink'], f'{what}: ray {r} alone'))
    med = float(np.median(worst))
    assert med <= bd['one_median'], f'{what}: median over {len(worst)} one-ray backwards {med:.3e} (bound {bd["one_median"]:.1e})'
    return med, max(worst)
