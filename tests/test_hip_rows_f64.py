"""Large batches against a float64 reference on SAMPLED ROWS (tests/rows_f64.py).

Every earlier comparison with an independent reference stops at 4096 rays; larger calls were checked by self-consistency only (determinism,
whole = halves, gradient additivity), which an error that the whole batch and its halves share passes.  Rays are independent, so a float64
restatement of a few rows R checks a HIP call of any size: the HIP module runs the whole N-ray batch (injected random numbers), and

  (a) every differentiable output of R's rows is compared with the float64 oracle on those rows (HIP's own depths teacher-forced);
  (b) one whole-batch backward with a seeded cotangent C that is non-zero on R only: all 48 parameter gradients against the float64
      gradient of sum(C * out) over R -- rel. L2 per tensor and the largest element;
  (c) one-ray cotangents, each in its own backward (the last ray; up to 8 rays that straddle a chunk boundary of the 256 x 256 weight-
      gradient class): a lost 32-point block is a 100 % error there.

R = the first and the last ray, up to 16 boundary-straddling rays of the 256 x 256 class (both levels), 64 seeded random rows.  The shapes
reach the planner's regimes no earlier comparison reached (tests/test_rows_f64_cpu.py pins the planner mirror): chunks that start past the
level's last point (4097 rays: 7 / 9 empty; 10 923 rays: 15 empty at the fine level) and the 256-chunk cap (10 923 x 192 = 2 097 216 points:
chunks of 8704 > 8192 points).  Bounds: rows_f64.BOUNDS, about twice the measured values (profiles/r07_rows_f64_measured.txt)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'vip-nerf_amd'), os.path.join(ROOT, 'vip-nerf_amd', 'src'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import rows_f64 as rf  # noqa: E402
from oracle import vipnerf_oracle as vo  # noqa: E402

# id: (precision, scene, frames (0: an empty rays_o2, V = 0), rays, workspace: 'plain' = capped at the call's own workspace (the plain
# backward, asserted), 'rerender' = capped to a re-rendering backward with a ragged last ray chunk)
CASES = {
    'fp32_fern_v1_4097': ('fp32', 'fern', 2, 4097, 'plain'),
    'fp32_fern_v1_10923': ('fp32', 'fern', 2, 10923, 'plain'),
    'fp32_dtu_v2_4097': ('fp32', 'dtu', 3, 4097, 'plain'),
    'fp32_fern_v3_4097': ('fp32', 'fern', 4, 4097, 'plain'),
    'fp32_fern_v0_4097': ('fp32', 'fern', 0, 4097, 'plain'),
    'fp16x3_fern_4097': ('fp16x3', 'fern', 2, 4097, 'plain'),
    'fp16x3_fern_10923': ('fp16x3', 'fern', 2, 10923, 'plain'),
    'fp16x3h_fern_4097': ('fp16x3h', 'fern', 2, 4097, 'plain'),
    'fp16x3h_fern_10923': ('fp16x3h', 'fern', 2, 10923, 'plain'),
    'bf16_dtu_16384': ('bf16', 'dtu', 3, 16384, 'plain'),
    'bf16_fern_3002': ('bf16', 'fern', 2, 3002, 'plain'),
    'fp16_dtu_16384': ('fp16', 'dtu', 3, 16384, 'plain'),
    'fp16_fern_3002': ('fp16', 'fern', 2, 3002, 'plain'),
    'fp32_fern_10923_rerender': ('fp32', 'fern', 2, 10923, 'rerender'),
}
NC, NF = 64, 128


def choose_rows(n, prec, seed):
    b = sorted(set(rf.boundary_rays(n, NC, prec) + rf.boundary_rays(n, NC + NF, prec)))
    if not b:                    # every boundary on a ray's edge (the 16-bit plan at 16 384 rays): the rays on both sides of each
        for S in (NC, NC + NF):
            nc, pts = rf.big_class_plan(n * S, prec)
            b += [r for k in range(1, nc) if k * pts < n * S for r in (k * pts // S - 1, k * pts // S)]
        b = sorted(set(b))
    if len(b) > 16:
        b = [b[int(i)] for i in np.linspace(0, len(b) - 1, 16).round()]
    g = np.random.default_rng(seed)
    rnd = g.choice(n, size=64, replace=False).tolist()
    return sorted(set([0, n - 1] + b + rnd)), b


def depth_ratio(h, ref, key, rows_b, ndc, eps):
    """the per-ray first-order bound of tests/test_hip_headline_size.py for the depth statistics (a weight error dw_i moves a ray's depth by
    dw_i |d_i - depth| / acc; NDC metric depths run to 1 / (1 - z)), with per-weight error eps w_i + 1e-3 eps -> max |h - ref| / bound"""
    lv = key.rsplit('_', 1)[1]
    is_ndc = key.endswith(f'ndc_{lv}')
    w, acc, z = ref[f'weights_{lv}'].detach(), ref[f'acc_{lv}'].detach(), ref[f'z_vals_{lv}'].detach()
    d = z if (is_ndc or not ndc) else vo.ndc_to_metric_depth(z, rows_b['rays_o'], rows_b['rays_d'])
    mean = ref[f"depth{'_ndc' if is_ndc else ''}_{lv}"].detach()
    dw = eps * w + 1e-3 * eps
    dev_i = (d - mean[:, None]).abs()
    tol_mean = eps * mean.abs() + (dw * dev_i).sum(-1) / (acc + 1e-6)
    r, o = ref[key].detach(), h.detach().cpu().double().reshape(ref[key].shape)
    assert torch.isfinite(o).all(), key
    if 'var' in key:
        tol = eps * r.abs() + (dw * dev_i ** 2).sum(-1) + 2 * (w * dev_i).sum(-1) * tol_mean + 0.1 * eps * float(r.abs().median())
    else:
        tol = tol_mean
    return float(((o - r).abs() / tol).max())


def _model(dev, prec, ndc, params, cap):
    import test_hip_parity as tp
    model, cfg = tp.make_model(dev, ndc, params)
    cfg['model']['hip_precision'] = prec
    cfg['model']['hip_max_workspace_bytes'] = int(cap)
    model.train()
    return model


def _hip_grads(model, rb, cts_dev):
    for t in model.parameters():
        t.grad = None
    out = model(rb)
    tot = 0
    for k, c in cts_dev.items():
        tot = tot + (out[k] * c).sum()
    tot.backward()
    g = {k: t.grad.detach().cpu().double() for k, t in model.named_parameters()}
    del out, tot
    return g


@pytest.mark.parametrize('case', list(CASES))
def test_rows_vs_float64(case):
    import test_hip_parity as tp
    from vipnerf_hip import autograd as ag, ops
    prec, scene, nf, n, ws = CASES[case]
    bd = rf.BOUNDS[prec]
    dev = torch.device('cuda:0')
    V = 0 if nf == 0 else nf - 1
    b = vo.synthetic_batch(n, 1701 + n, scene=scene, nf=max(nf, 2))
    params = vo.init_params(1702, scale=1.6)
    rng = vo.synthetic_rng(n, NC, NF, 1703)
    cfg_o = {'ndc': b['ndc'], 'n_coarse': NC, 'n_fine': NF, 'noise_std': 1.0}
    rows, brays = choose_rows(n, prec, 1704)
    assert len(rows) <= 600

    # the workspace regime, asserted
    c = ops.make_config(b['ndc'], NC, NF, V, True, save_acts=True, precision=ops.PRECISIONS[prec])
    ab, bb = ops.query_workspace(c, n)
    if ws == 'plain':
        cap = ab + bb
        assert ag._recompute_chunk(ag.RenderState(c, {}, None, None, cap), n, ab, bb, dev) == 0
    else:
        cap = sum(ops.query_workspace(c, 4096)) + (1 << 20)
        chunk = ag._recompute_chunk(ag.RenderState(c, {}, None, None, cap), n, ab, bb, dev)
        assert 0 < chunk < n and n % chunk, chunk                      # a re-rendering backward with a ragged last ray chunk
    Pf = n * (NC + NF)
    if n == 10923:
        assert rf.wgrad_chunks(Pf) == rf.WGRAD_MAX_CHUNKS and rf.wgrad_chunk_pts(Pf) > rf.WGRAD_CHUNK_PTS          # the 256-chunk cap
        if prec not in rf.T16:
            assert rf.empty_chunks(Pf, prec) == 15
    if n == 4097 and prec not in rf.T16:
        assert rf.empty_chunks(n * NC, prec) == 7 and rf.empty_chunks(Pf, prec) == 9

    model = _model(dev, prec, b['ndc'], params, cap)
    model.injected_rng = {k: v.to(dev) for k, v in rng.items()}
    rb = tp.ref_batch(b, dev, 40000)
    if nf == 0:
        rb['rays_o2'] = torch.zeros(n, 0, 3, device=dev)
    with torch.no_grad():
        out = model(rb)
    keys = rf.diff_keys(out)
    idx = torch.as_tensor(rows)
    zc, zf = out['z_vals_coarse'][idx.to(dev)].cpu(), out['z_vals_fine'][idx.to(dev)].cpu()
    p64, ref = rf.reference_rows(params, b, rng, rows, zc, zf, cfg_o, sec_views=nf > 0)
    keys = [k for k in keys if k in ref]
    assert 'rgb_fine' in keys and ('visibility2_fine' in keys) == (V > 0)

    # (a) outputs
    rows_b = rf.rows_batch(b, rows)
    worst_out, worst_depth = (0.0, ''), (0.0, '')
    for k in keys:
        h = out[k][idx.to(dev)]
        if k.startswith('depth'):
            r = depth_ratio(h, ref, k, rows_b, b['ndc'], bd['depth_eps'])
            worst_depth = max(worst_depth, (r, k))
        else:
            e = rf.output_error(h, ref[k])
            worst_out = max(worst_out, (e, k))
    shapes = {k: tuple(out[k].shape) for k in keys}
    del out

    # (b) the R-row backward
    names = [k for k, _ in model.named_parameters()]
    cts = rf.cotangents(ref, keys, shapes, rows, n, seed=1705)
    g64 = rf.reference_grads(p64, ref, cts, rows, names, retain=True)
    gh = _hip_grads(model, rb, {k: v.to(dev) for k, v in cts.items()})
    errs_b = {k: rf.grad_error(gh[k].numpy(), g64[k].numpy()) for k in names if float(g64[k].abs().max()) > 0}
    # (c) one-ray backwards
    singles = [n - 1] + brays[:8]
    errs_c = []
    for r in dict.fromkeys(singles):
        c1 = rf.single_row(cts, r)
        g1 = rf.reference_grads(p64, ref, c1, rows, names, retain=True)
        h1 = _hip_grads(model, rb, {k: v.to(dev) for k, v in c1.items()})
        errs_c.append((r, g1, h1))
    del model
    torch.cuda.empty_cache()

    if os.environ.get('VIPNERF_ROWS_LOG'):               # the per-tensor record of a measurement pass (profiles/r07_rows_f64_measured.txt)
        with open(os.environ['VIPNERF_ROWS_LOG'], 'a') as f:
            for k in names:
                if k in errs_b:
                    f.write('%-28s R rows   %-44s l2 %.3e max %.3e\n' % (case, k, *errs_b[k]))
            for r, g1, h1 in errs_c:
                e1 = [(rf.grad_error(h1[k].numpy(), g1[k].numpy())[0], k) for k in names if float(g1[k].abs().max()) > 0]
                f.write('%-28s ray %-5d worst %-44s l2 %.3e\n' % (case, r, max(e1)[1], max(e1)[0]))
    wb = max(errs_b.values())
    per_ray = [max(rf.grad_error(h1[k].numpy(), g1[k].numpy())[0] for k in names if float(g1[k].abs().max()) > 0) for _, g1, h1 in errs_c]
    wc, mc = max(per_ray), float(np.median(per_ray))
    print(f'{case}: {len(rows)} rows ({len(brays)} boundary rays); outputs worst {worst_out[0]:.2e} ({worst_out[1]}, ratio {worst_out[0] / bd["out"]:.2f}), '
          f'depth statistics {worst_depth[0]:.2f} x their first-order bound ({worst_depth[1]}); R-row gradients worst rel L2 {wb[0]:.2e} '
          f'(max-element {max(e[1] for e in errs_b.values()):.2e}, ratio {wb[0] / bd["grad"]:.2f}); one-ray gradients ({len(errs_c)}) worst rel L2 {wc:.2e} '
          f'(ratio {wc / bd["one_kink"]:.2f}), median {mc:.2e} (ratio {mc / bd["one_median"]:.2f})')
    assert worst_out[0] <= bd['out'], f'{case}: output {worst_out[1]} {worst_out[0]:.3e} (bound {bd["out"]:.1e})'
    assert worst_depth[0] <= 1.0, f'{case}: {worst_depth[1]} {worst_depth[0]:.2f} x its first-order bound'
    rf.check_grads(gh, g64, bd['grad'], f'{case} R rows')
    rf.check_one_rays([(r, h1, g1) for r, g1, h1 in errs_c], bd, case)
