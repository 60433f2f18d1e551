"""CPU side of the float64 row reference (tests/rows_f64.py): the planner mirror pinned against the library's own workspace query, the
oracle's float64 mode, and the bounds of tests/test_hip_rows_f64.py shown able to fail (modelled on tests/test_tolerances_cpu.py)."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'vip-nerf_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import rows_f64 as rf  # noqa: E402
from oracle import vipnerf_oracle as vo  # noqa: E402

# (rays, samples per ray): the cases of tests/test_hip_rows_f64.py and both sides of the 32 768 / 262 144 / 2 097 152-point regime edges
SHAPES = [(4097, 64), (4097, 192), (10923, 64), (10923, 192), (16384, 64), (16384, 192), (3002, 64), (3002, 192),
          (512, 64), (511, 64), (513, 64), (32767, 1 + 1), (4096, 64), (4095, 64), (2047, 128), (2049, 128),
          (16384, 128), (16383, 128), (16385, 128), (10922, 192), (32768, 64), (32769, 64), (1, 5), (37, 101), (0, 64)]


@pytest.mark.parametrize('V', [0, 1, 3])
def test_planner_mirror_is_the_library_workspace(V):
    """vipnerf_query_workspace folds wgrad_partial_total(P, V) into the backward scratch (bwd_layout): a coarse-only fp32 call of N rays x S
    samples reports bwd_layout(N S, V).total floats -- the mirror must give the same number at every shape, regime edges included."""
    from vipnerf_hip import _lib, ops
    lib = _lib.load()
    a, b = C.c_size_t(), C.c_size_t()
    for n, S in SHAPES:
        cfg = ops.make_config(True, S, 0, V, True, save_acts=True)
        assert lib.vipnerf_query_workspace(C.byref(cfg), n, C.byref(a), C.byref(b)) == 0, (n, S)
        assert b.value == 4 * rf.bwd_layout_total(n * S, V), (n, S, V, b.value, 4 * rf.bwd_layout_total(n * S, V))


def test_planner_regimes():
    """the regimes the row tests are built to reach"""
    # 4097 x 64: 64 chunks of 4608 points, 7 of them empty; the fine level 128 chunks of 6656, 9 empty
    assert rf.big_class_plan(4097 * 64, 'fp32') == (64, 4608) and rf.empty_chunks(4097 * 64, 'fp32') == 7
    assert rf.big_class_plan(4097 * 192, 'fp32') == (128, 6656) and rf.empty_chunks(4097 * 192, 'fp32') == 9
    # 10 923 x 192 = 2 097 216 points: past the 256-chunk cap -- chunks of 8704 > 8192 points, 15 empty
    P = 10923 * 192
    assert P > 2097152 and rf.big_class_plan(P, 'fp32') == (256, 8704) and rf.empty_chunks(P, 'fp16x3') == 15
    assert rf.wgrad_chunk_pts(2097152) == 8192 and rf.wgrad_chunk_pts(P) > 8192
    # below 32 768 points and at exact multiples there is no empty chunk (every earlier oracle comparison)
    for n, S in ((4096, 64), (4096, 192), (1024, 64), (1024, 192), (511, 64)):
        assert rf.empty_chunks(n * S, 'fp32') == 0
    # the 16-bit plan re-derives its chunk count where a level has more than one round of workgroups (more than 32 chunks): never empty
    # there; below, it keeps the shared plan, empty chunks included (513 x 64: 32 chunks of 1536 points, 10 empty)
    for n, S in SHAPES:
        for prec in rf.T16:
            if rf.wgrad_chunks(n * S) > 32:
                assert rf.empty_chunks(n * S, prec) == 0
    assert rf.empty_chunks(513 * 64, 'bf16') == 10
    # boundary rays: a boundary inside a ray (4097 x 64: 4608 / 64 = 72 is whole -- none; 10 923 x 192: 8704 / 192 is not)
    assert rf.boundary_rays(4097, 64, 'fp32') == []
    b = rf.boundary_rays(10923, 192, 'fp32')
    inner = [k * 8704 for k in range(1, 256) if k * 8704 < P and (k * 8704) % 192]      # 8704 = 45 1/3 rays: every third boundary is a ray's edge
    assert len(b) == len(inner) == 160 and all(r * 192 < e < (r + 1) * 192 for e, r in zip(inner, b))
    assert len(rf.boundary_rays(3002, 192, 'fp16')) > 0 and len(rf.boundary_rays(4097, 192, 'fp32')) > 0


def _small_case():
    b = vo.synthetic_batch(48, 71, scene='fern', nf=2)
    params = vo.init_params(72, scale=1.6)
    rng = vo.synthetic_rng(48, 64, 128, 73)
    cfg_o = {'ndc': True, 'n_coarse': 64, 'n_fine': 128, 'noise_std': 1.0}
    return b, params, rng, cfg_o


def test_oracle_float64_computes_in_float64():
    """No step of render_rays / composite / the losses makes a constant or an intermediate in the default dtype: the float64 run is the same
    bit for bit whatever the default dtype is, every floating output is float64, and float32 inputs still give float32."""
    b, params, rng, cfg_o = _small_case()
    rows = list(range(0, 48, 3))
    with torch.no_grad():
        ref32 = vo.render_rays(vo.params_to_torch(params), b, cfg_o, rng, train=True, sec_views=True)
    z_c, z_f = ref32['z_vals_coarse'][rows], ref32['z_vals_fine'][rows]
    lcfg = [{'name': 'MSE01', 'weight': 1}, {'name': 'VisibilityLoss01', 'weight': 0.1},
            {'name': 'VisibilityPriorLoss01', 'iter_weights': {'0': 0, '30000': 0.001}}, {'name': 'SparseDepthMSE01', 'weight': 0.1}]
    runs = []
    old = torch.get_default_dtype()
    try:
        for dt in (torch.float32, torch.float64):
            torch.set_default_dtype(dt)
            with torch.no_grad():
                _, out = rf.reference_rows(params, b, rng, rows, z_c, z_f, cfg_o)
                sub = rf.rows_batch(b, rows)
                sub.pop('visibility_prior_masks')           # the prior's all-ones default weights
                loss = vo.total_loss(sub, out, lcfg, 40000)
            runs.append((out, loss))
    finally:
        torch.set_default_dtype(old)
    for k, v in runs[0][0].items():
        if v.is_floating_point():
            assert v.dtype == torch.float64, k
            assert torch.equal(v, runs[1][0][k]), k
    for k, v in runs[0][1].items():
        assert torch.as_tensor(v).dtype == torch.float64 and torch.equal(torch.as_tensor(v), torch.as_tensor(runs[1][1][k])), k
    assert all(v.dtype == torch.float32 for v in ref32.values() if v.is_floating_point())
    # the float64 outputs are the float32 ones to float32 rounding (a check of the upcast and of the teacher forcing)
    for k in ('rgb_fine', 'acc_coarse', 'weights_fine', 'visibility2_fine'):
        assert float((runs[0][0][k] - ref32[k][rows].double()).abs().max()) <= 1e-5, k
    # teacher-forced coarse depths equal to the drawn ones change nothing
    with torch.no_grad():
        forced = vo.render_rays(vo.params_to_torch(params), b, cfg_o, dict(rng, z_coarse=ref32['z_vals_coarse']), train=True, sec_views=True)
    assert all(torch.equal(forced[k], ref32[k]) for k in ref32)


# ------------------------------------------------------------------------------------------------ the bounds can fail
def _reference_with_cotangent(monkeypatch=None, drop=None):
    """float64 gradient of sum(C * out) over R = 12 rows of a 48-ray batch; drop = (row position in R, level, first point): that ray's 32-point
    block of the level enters the gradient with its MLP parameters detached -- exactly what a weight-gradient GEMM that loses the block computes"""
    b, params, rng, cfg_o = _small_case()
    rows = [0, 5, 9, 13, 17, 22, 26, 30, 35, 39, 44, 47]
    with torch.no_grad():
        ref32 = vo.render_rays(vo.params_to_torch(params), b, cfg_o, rng, train=True, sec_views=True)
    if drop is not None:
        j, level, p0 = drop
        S = 64 if level == 'coarse' else 192
        real = vo.mlp_forward

        def mlp(p, lv, pts, *a, **kw):
            if lv != level:
                return real(p, lv, pts, *a, **kw)
            q = {k: v.detach() for k, v in p.items()}
            lo, hi = j * S + p0, j * S + p0 + 32
            cut = lambda t, s, e: None if t is None else t[s:e]
            parts = [real(p, lv, pts[:lo], *[cut(t, 0, lo) for t in a], **kw), real(q, lv, pts[lo:hi], *[cut(t, lo, hi) for t in a], **kw),
                     real(p, lv, pts[hi:], *[cut(t, hi, None) for t in a], **kw)]
            return {k: torch.cat([x[k] for x in parts], 0) for k in parts[0]}
        monkeypatch.setattr(vo, 'mlp_forward', mlp)
    p, out = rf.reference_rows(params, b, rng, rows, ref32['z_vals_coarse'][rows], ref32['z_vals_fine'][rows], cfg_o)
    keys = [k for k in rf.diff_keys(out)]
    shapes = {k: (48,) + tuple(out[k].shape[1:]) for k in keys}
    cts = rf.cotangents(out, keys, shapes, rows, 48, seed=5)
    names = sorted(params)
    g = rf.reference_grads(p, out, cts, rows, names, retain=True)
    # the last ray alone, relative to R: its cotangent only
    g1 = rf.reference_grads(p, out, rf.single_row(cts, rows[-1]), rows, names)
    return g, g1, names


def test_the_row_bounds_fail_when_they_must(monkeypatch):
    """Each perturbation is caught by the checks of tests/test_hip_rows_f64.py at their bounds (rows_f64.BOUNDS), rounding passes:
      * one row's contribution missing from the R-row gradient: check (b), every fp32-grade class;
      * a relative error of 1e-3 on every gradient: the median of the one-ray backwards (c), fp32 and fp16x3 -- the R-row bound (b) sits above
        1e-3 because of kink events (one ray of R at a ReLU's rounding level), the median of the one-ray backwards does not;
      * one 32-point block of one ray lost: the one-ray check (c), every class but bf16 (whose one-ray bound, 0.45, is above a block's share);
      * the ray lost altogether: (c), every class."""
    g, g_last, names = _reference_with_cotangent()
    fp32_grade = ('fp32', 'fp16x3', 'fp16x3h')
    rays = lambda got, ref: [(r, got, ref) for r in range(9)]          # nine one-ray backwards alike
    for prec in fp32_grade:
        bd = rf.BOUNDS[prec]
        with pytest.raises(AssertionError, match='rel L2'):
            rf.check_grads({k: g[k] - g_last[k] for k in names}, g, bd['grad'], f'{prec}: the last row dropped')
        if prec != 'fp16x3h':                                 # (fp16x3h's gradients are of their own class: median 6.3e-4 measured)
            with pytest.raises(AssertionError, match='median'):
                rf.check_one_rays(rays({k: g_last[k] * (1 + 1e-3) for k in names}, g_last), bd, f'{prec}: 1e-3 injected')
        # rounding-level differences pass: the float32 rounding of the gradient, and 1e-7 relative
        for what, f in (('float32 rounding', lambda t: t.float()), ('1e-7', lambda t: t * (1 + 1e-7))):
            rf.check_grads({k: f(g[k]) for k in names}, g, bd['grad'], f'{prec}: {what}')
            rf.check_one_rays(rays({k: f(g_last[k]) for k in names}, g_last), bd, f'{prec}: {what}')
    for prec, bd in rf.BOUNDS.items():
        with pytest.raises(AssertionError, match='no gradient'):
            rf.check_one_rays(rays({k: torch.zeros_like(g_last[k]) for k in names}, g_last), bd, f'{prec}: the ray lost')
        with pytest.raises(AssertionError, match='rel L2'):
            rf.check_one_rays(rays({k: 0.5 * g_last[k] for k in names}, g_last), bd, f'{prec}: half the ray lost')
    # one 32-point block of one ray lost (the last row's last fine block; and a coarse block in the middle of a row of R)
    for drop in ((11, 'fine', 160), (6, 'coarse', 32)):
        with monkeypatch.context() as mp:
            gd, gd_last, _ = _reference_with_cotangent(mp, drop)
        if drop[0] == 11:
            for prec, bd in rf.BOUNDS.items():
                if prec != 'bf16':
                    with pytest.raises(AssertionError, match='rel L2'):
                        rf.check_one_rays([(47, gd_last, g_last)] + rays(g_last, g_last), bd, f'{prec}: block {drop} lost (one ray)')
        errs = [rf.grad_error(gd[k].numpy(), g[k].numpy())[0] for k in names if float(g[k].abs().max()) > 0]
        assert max(errs) > 1e-3, (drop, max(errs))          # the block's share of the R-row gradient (R = 12 rows here) is visible
