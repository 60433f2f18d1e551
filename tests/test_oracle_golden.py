"""The CPU oracle (oracle/vipnerf_oracle.py) against the golden vectors captured from the real reference
(oracle/gen_golden.py).  CPU only.  Tolerances are written per check; indices are compared bit-exactly."""
import os

import numpy as np
import pytest
import torch

from oracle import vipnerf_oracle as vo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name):
    """One fixture: <name>.npz, or the <name>.part<i>.npz files a large one is written as (oracle/gen_golden.py::npz)."""
    import glob
    files = [os.path.join(GOLD, name + '.npz')]
    if not os.path.exists(files[0]):
        files = sorted(glob.glob(os.path.join(GOLD, name + '.part*.npz')), key=lambda f: int(f.rsplit('.part', 1)[1][:-4]))
    assert files, name
    return {k: v for f in files for k, v in np.load(f, allow_pickle=False).items()}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def close(a, b, rtol=1e-5, atol=1e-6):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    np.testing.assert_allclose(a, np.asarray(b), rtol=rtol, atol=atol)


def digest(t):
    f = t.detach().reshape(-1).double()
    n = f.numel()
    idx = (torch.arange(192, dtype=torch.long) * 7919) % n
    return torch.cat([f.sum()[None], f.norm()[None], f[:64] if n >= 64 else torch.cat([f, f.new_zeros(64 - n)]),
                      f[idx]]).numpy()


def test_f1_sample_pdf_indices_bit_exact():
    g = load('f1_sample_pdf')
    s, inds = vo.sample_pdf(T(g['bins']), T(g['weights']), T(g['u']))
    assert np.array_equal(inds.numpy(), g['inds_rand'])            # bit-exact sample indices
    close(s, g['samples_rand'], rtol=0, atol=0)
    u_det = torch.linspace(0., 1., steps=128).expand(g['bins'].shape[0], 128)
    s, inds = vo.sample_pdf(T(g['bins']), T(g['weights']), u_det)
    assert np.array_equal(inds.numpy(), g['inds_det'])
    close(s, g['samples_det'], rtol=0, atol=0)


@pytest.mark.parametrize('V', [1, 2])
def test_f2_mlp_forward(V):
    g = load(f'f2_mlp_v{V}')
    p = vo.params_to_torch(vo.init_params(int(g['seed']), levels=('coarse',)))
    close(vo.positional_encode(T(g['pts']), 10), g['enc_pts'], rtol=0, atol=0)
    for mode, noise in (('train', T(g['noise'])), ('eval', None)):
        o = vo.mlp_forward(p, 'coarse', T(g['pts']), T(g['view_dirs']), T(g['view_dirs2']), noise)
        close(o['sigma'], g[f'sigma_{mode}'], rtol=1e-5, atol=1e-6)
        close(o['rgb'], g[f'rgb_{mode}'], rtol=1e-5, atol=1e-6)
        close(o['visibility'], g[f'vis_{mode}'], rtol=1e-5, atol=1e-6)
        close(o['visibility2'], g[f'vis2_{mode}'], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('scene', ['fern', 'dtu'])
def test_f3_composite(scene):
    g = load(f'f3_composite_{scene}')
    ndc = bool(g['ndc'])
    net = {'sigma': T(g['sigma']), 'rgb': T(g['rgb']), 'visibility2': T(g['vis2'])}
    z, o, d = T(g['z']), T(g['rays_o']), T(g['rays_d'])
    dn = T(g['rays_d_ndc']) if ndc else d
    out = vo.composite(net, z, dn, ndc, o, d)
    for k in ('rgb', 'acc', 'alpha', 'visibility', 'weights', 'depth', 'depth_var', 'visibility2') + \
            (('depth_ndc', 'depth_var_ndc') if ndc else ()):
        close(out[k], g['out_' + k], rtol=1e-6, atol=1e-7)
    if ndc:
        close(vo.ndc_to_metric_depth(z, o, d), g['metric_depth'], rtol=0, atol=0)
    close(vo.secondary_dirs(z, o, d, T(g['rays_o2']), ndc), g['dirs2'], rtol=1e-6, atol=1e-7)


def _cfg(ndc, n_fine=128, depth=8):
    return {'ndc': ndc, 'n_coarse': 64, 'n_fine': n_fine, 'depth': depth, 'noise_std': 1.0}


def _check_outputs(out, g, levels, rtol, atol):
    for lv in levels:
        for k in ['rgb', 'acc', 'depth', 'depth_var', 'depth_ndc', 'depth_var_ndc', 'visibility2', 'z_vals',
                  'alpha', 'visibility', 'weights', 'raw_sigma', 'raw_rgb', 'raw_visibility', 'raw_visibility2']:
            kk = f'out_{k}_{lv}'
            if kk in g:
                close(out[f'{k}_{lv}'], g[kk], rtol=rtol, atol=atol)


def test_f4_eval_render():
    g = load('f4_eval_fern')
    b = vo.synthetic_batch(int(g['n']), int(g['seed_batch']), scene='fern', nf=2)
    p = vo.params_to_torch(vo.init_params(int(g['seed_params']), scale=float(g['scale_params']),
                                          sigma_bias=float(g['sigma_bias'])))
    with torch.no_grad():
        out = vo.render_rays(p, b, _cfg(True), None, train=False, sec_views=True)
        plain = vo.render_rays(p, b, _cfg(True), None, train=False, sec_views=False)
    _check_outputs(out, g, ('coarse', 'fine'), rtol=2e-5, atol=2e-6)
    # the reference's plain eval key set (retraw=False drops z_vals/visibility/weights/raw_*, keeps alpha)
    for k in g['keys_plain']:
        close(plain[str(k)], g['plain_' + str(k)], rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize('tag', ['llff', 'realestate', 'dtu', 'toy', 'dtu4wl', 'toy_rgbtrunk', 'dtu_novis', 'fern_plain'])
def test_f5_train_step(tag):
    """One training step of the reference, captured: outputs, losses, parameter gradients, one Adam step.  The last three are the head
    variants no shipped config uses (mlp `view_dependent_rgb` / `predict_visibility` = False, VipNeRF01.py:467-491): rgb from the trunk
    head, no visibility (MSE only), neither (no view branch)."""
    g = load(f'f5_train_{tag}')
    heads = dict(view_dep_rgb=bool(g['view_dep_rgb']) if 'view_dep_rgb' in g else True, predict_vis=bool(g['predict_vis']) if 'predict_vis' in g else True)
    depth, width, n_fine = int(g['depth']), int(g['width']), int(g['n_fine'])
    levels = ('coarse', 'fine') if n_fine > 0 else ('coarse',)
    b = vo.synthetic_batch(int(g['n']), int(g['seed_batch']), scene=str(g['scene']), nf=int(g['nf']),
                           n_sparse=int(g['n_sparse']))
    params = vo.init_params(int(g['seed_params']), depth=depth, width=width, levels=levels,
                            scale=float(g['scale_params']), **heads)
    p = vo.params_to_torch(params, requires_grad=True)
    rng = {k[4:]: T(v) for k, v in g.items() if k.startswith('rng_')}
    cfg = _cfg(b['ndc'], n_fine, depth)
    cfg.update(white_bkgd=bool(g.get('white_bkgd', False)), lindisp=bool(g.get('lindisp', False)), **heads)   # 'dtu4wl': V = 3, both on
    out = vo.render_rays(p, b, cfg, rng, train=True, sec_views=True)
    _check_outputs(out, g, levels, rtol=2e-5, atol=2e-6)
    if 'out_keys' in g:                          # the variant's key set is the reference's (raw_rgb_view_independent_*, no visibility2_* ...)
        assert {str(k) for k in g['out_keys']} <= set(out.keys()), sorted({str(k) for k in g['out_keys']} - set(out.keys()))
        assert not [k for k in out if ('visibility2' in k or 'raw_visibility' in k or 'view_' in k) and k not in {str(q) for q in g['out_keys']}]
    lcfg = [{'name': 'MSE01', 'weight': 1}, {'name': 'VisibilityLoss01', 'weight': 0.1},
            {'name': 'VisibilityPriorLoss01', 'iter_weights': {'0': 0, '30000': 0.001}}][:3 if heads['predict_vis'] else 1]
    if int(g['n_sparse']) > 0:
        lcfg.append({'name': 'SparseDepthMSE01', 'weight': 0.1})
    for nm, it in (('l40k', 40000), ('l0', 0)):
        lv = vo.total_loss(b, out, lcfg, it, levels)
        for k, v in lv.items():
            close(v, g[f'{nm}_{k}'], rtol=1e-5, atol=1e-7)
    vo.total_loss(b, out, lcfg, 40000, levels)['TotalLoss'].backward()
    opt = torch.optim.Adam(list(p.values()), lr=5e-4, betas=(0.9, 0.999))
    for k, t in p.items():
        gd = g['gdig_' + k]
        scale = max(abs(gd[1]), 1e-12)          # l2 norm of the reference grad
        np.testing.assert_allclose(digest(t.grad), gd, rtol=1e-3, atol=2e-5 * scale + 1e-9)
        if 'grad_' + k in g:
            np.testing.assert_allclose(t.grad.numpy(), g['grad_' + k], rtol=1e-3, atol=2e-5 * scale + 1e-9)
    opt.step()
    for k, t in p.items():
        # Adam's first step moves every weight by ~lr*sign(g); where |g| is at rounding level the sign is
        # not reproducible, so compare with an absolute tolerance of one step
        np.testing.assert_allclose(digest(t)[2:], g['adig_' + k][2:], rtol=0, atol=1.1e-3)
        np.testing.assert_allclose(digest(t)[1], g['adig_' + k][1], rtol=1e-4)


def test_f9_trajectory():
    """F9: eight iterations of the reference's Trainer.train_one_iter under its lr decayer, the visibility-prior weight switching on at
    30000 inside the window.  The oracle, fed each iteration's recorded draws and teacher-forced with its fine depths, stepped by torch's
    Adam, must follow the reference's losses to 1e-5 and its parameters to 5e-6 (measured: losses 2.3e-7, parameters 2.8e-6 where the
    gradient stayed above rounding level, 9.2e-6 elsewhere).  Free-running (its own fine depths from parameters that carry rounding-level
    differences after the first step) the fine colour stays within north_star's 1e-4 (measured 5.2e-5: the sampler's conditioning)."""
    g = load('f9_trajectory_fern')
    n, first, iters = int(g['n']), int(g['first_iter']), int(g['iters'])
    p = vo.params_to_torch(vo.init_params(int(g['seed_params']), scale=float(g['scale_params'])), requires_grad=True)
    opt = torch.optim.Adam(list(p.values()), lr=5e-4, betas=(0.9, 0.999))
    lcfg = [{'name': 'MSE01', 'weight': 1}, {'name': 'VisibilityLoss01', 'weight': 0.1},
            {'name': 'VisibilityPriorLoss01', 'iter_weights': {'0': 0, '30000': 0.001}}]
    cfg = _cfg(True, 128, 8)
    switched = []
    for i in range(iters):
        it = first + i
        lr = 5e-4 * 0.1 ** (it / 250000.0)                     # NeRFLearningRateDecayer01.py:19-23
        assert lr == float(g[f'it{i}_lr']), (lr, float(g[f'it{i}_lr']))
        for grp in opt.param_groups:
            grp['lr'] = lr
        b = vo.synthetic_batch(n, int(g['seed']) + 10 + i, scene='fern', nf=2)
        rng = {k[len(f'it{i}_rng_'):]: T(v) for k, v in g.items() if k.startswith(f'it{i}_rng_')}
        with torch.no_grad():
            free = vo.render_rays(p, b, cfg, rng, train=True, sec_views=True)
        close(free['rgb_fine'], g[f'it{i}_rgb_fine'], rtol=0, atol=1e-4)
        rng['z_fine'] = T(g[f'it{i}_z_vals_fine'])
        opt.zero_grad(set_to_none=True)
        out = vo.render_rays(p, b, cfg, rng, train=True, sec_views=True)
        close(out['rgb_fine'], g[f'it{i}_rgb_fine'], rtol=2e-5, atol=2e-6)
        lv = vo.total_loss(b, out, lcfg, it)
        for k, v in lv.items():
            close(v.detach(), g[f'it{i}_loss_{k}'], rtol=1e-5, atol=1e-7)
        switched.append(vo.schedule_weight(lcfg[2], it))
        lv['TotalLoss'].backward()
        opt.step()
        for k, t in p.items():
            np.testing.assert_allclose(digest(t)[1], g[f'it{i}_pdig_{k}'][1], rtol=1e-5, err_msg=f'iteration {i}: |{k}|')
    assert switched == [0, 0, 0, 0, 0.001, 0.001, 0.001, 0.001]
    for k, t in p.items():
        after, ref, firm = digest(t)[2:], g['adig_' + k][2:], g['gmin_' + k] > 1e-6
        np.testing.assert_allclose(after[firm], ref[firm], rtol=0, atol=5e-6, err_msg=f'{k} after {iters} iterations')
        np.testing.assert_allclose(after[~firm], ref[~firm], rtol=0, atol=2e-5, err_msg=f'{k} (gradients at rounding level in some iteration)')
        if 'after_' + k in g:
            np.testing.assert_allclose(t.detach().numpy(), g['after_' + k], rtol=0, atol=2e-5, err_msg=k)


def test_f6_raygen_and_postprocess():
    """oracle/raygen_oracle.py against the reference's DataPreprocessor: bit-exact."""
    from oracle import raygen_oracle as ro
    g = load('f6_raygen')
    res = tuple(int(v) for v in g['resolution'])
    for i in range(3):
        o, d = ro.get_rays(res, g['intrinsic'], g['poses'][i])
        assert np.array_equal(o, g[f'rays_o_{i}']) and np.array_equal(d, g[f'rays_d_{i}'])
        assert np.array_equal(ro.get_view_dirs(d), g[f'view_dirs_{i}'])
        on, dn = ro.get_ndc_rays(o, d, res, g['intrinsic'], float(g['near']))
        assert np.array_equal(on, g[f'rays_o_ndc_{i}']) and np.array_equal(dn, g[f'rays_d_ndc_{i}'])
    assert np.array_equal(ro.post_process_image(g['pp_rgb'].reshape(res[0], res[1], 3)), g['pp_image'])
    assert np.array_equal(ro.post_process_depth(g['pp_depth'].reshape(res)), g['pp_depth_out'])


def test_f7_visibility_prior_generator():
    from oracle import psv_oracle as po
    g = load('f7_visibility_prior')
    for a, b, ea, eb, key in (('frame1', 'frame2', 'E1', 'E2', 'weights12'), ('frame2', 'frame1', 'E2', 'E1', 'weights21')):
        w = po.compute_weights(g[a], g[b], g[ea], g[eb], g['K'], g['K'], float(g['min_depth']), float(g['max_depth']),
                               int(g['n_planes']), float(g['temperature']))
        np.testing.assert_allclose(w, g[key], rtol=1e-11, atol=1e-13)
        assert np.array_equal(w > 0.5, g[key] > 0.5)


def test_committed_goldens_are_what_the_reference_produces():
    """Every committed fixture is what the reference produced: same files, same keys, every array bit for bit against the digests
    (dtype, shape, sha256) that `oracle/check_goldens.py --write-digests` recorded from a fresh run of the reference's own code
    (tests/golden/reference_digests.json) -- a fixture edited or regenerated without the reference fails here."""
    import json
    from oracle import check_goldens as cg
    recorded = json.load(open(cg.DIGESTS))
    now = cg.digests(GOLD)
    assert sorted(now) == sorted(recorded), sorted(set(now) ^ set(recorded))
    for f in recorded:
        assert now[f] == recorded[f], (f, sorted(k for k in recorded[f] if now[f].get(k) != recorded[f][k])[:8])
