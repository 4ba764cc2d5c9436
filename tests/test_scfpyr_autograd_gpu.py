"""GPU: autograd through SCFpyr_PyTorch.build and .reconstruct (mm_scfpyr_build_adjoint / mm_scfpyr_reconstruct_adjoint,
csrc/scfpyr.hip) -- parity with the real reference's torch-autograd gradients (tests/golden/scfpyr_grad.npz), the adjoint
(dot-product) identity, gradcheck / gradgradcheck, the forward unchanged on the grad path, upstream gradients that are
missing, expanded or non-contiguous, handle re-resolution, determinism, the C ABI error paths and the general
Phase_Difference_Extractor.build_pyramid.  The fixture's cotangents are regenerated (scfpyr_grad_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import scfpyr_grad_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _pyr(height, nbands, dev, precision):
    from mimamo_net_amd.scfpyr import SCFpyr_PyTorch
    return SCFpyr_PyTorch(height=height, nbands=nbands, scale_factor=2, device=dev, precision=precision)


def _flatten(coeff):
    return [coeff[0]] + [b for level in coeff[1:-1] for b in level] + [coeff[-1]]


def _nest(flat, height, nbands):
    return [flat[0]] + [list(flat[1 + l * nbands:1 + (l + 1) * nbands]) for l in range(height - 2)] + [flat[-1]]


def _rand(shape, seed, dev, dt=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).to(dev, dt)


def _dot(a, b):
    return sum(float((x.detach().double() * y.detach().double()).sum()) for x, y in zip(a, b))


def _norm(a):
    return float(torch.sqrt(sum((x.detach().double() ** 2).sum() for x in a)))


@pytest.mark.parametrize("tag", sorted(cases.CASES))
@pytest.mark.parametrize("precision", [32, 64])
def test_build_gradient_matches_reference(pkg, golden, dev, tag, precision):
    g = golden("scfpyr_grad")
    cases.check_cfg(g, tag)
    size, height, nbands, n = cases.CASES[tag][:4]
    dt = torch.float32 if precision == 32 else torch.float64
    x = torch.zeros((n, 1, size, size), dtype=dt, device=dev, requires_grad=True)
    flat = _flatten(_pyr(height, nbands, dev, precision).build(x))
    w = [torch.from_numpy(c).to(dev, dt) for c in cases.coeff_cotangents(tag)]
    (gx,) = torch.autograd.grad(flat, x, grad_outputs=w)
    assert gx.dtype == dt and tuple(gx.shape) == (n, 1, size, size)
    want = g[tag + "_gx64"]
    err = np.abs(gx.double().cpu().numpy() - want).max()
    if precision == 64:
        assert err <= 1e-12 * max(1.0, np.abs(want).max()), err
    else:   # float64 inside: no worse than the reference's own fp32 gradient
        assert err <= float(g[tag + "_gx_gap32"]), (err, float(g[tag + "_gx_gap32"]))


@pytest.mark.parametrize("tag", cases.RECON_CASES)
@pytest.mark.parametrize("precision", [32, 64])
def test_reconstruct_gradient_matches_reference(pkg, golden, dev, tag, precision):
    g = golden("scfpyr_grad")
    cases.check_cfg(g, tag)
    size, height, nbands, n = cases.CASES[tag][:4]
    dt = torch.float32 if precision == 32 else torch.float64
    flat = [torch.zeros(shp, dtype=dt, device=dev, requires_grad=True) for shp in cases.shapes(size, height, nbands, n)]
    out = _pyr(height, nbands, dev, precision).reconstruct(_nest(flat, height, nbands))
    y = torch.from_numpy(cases.image_cotangent(tag)).to(dev, dt)
    grads = torch.autograd.grad(out, flat, grad_outputs=y)
    gap = float(g[tag + "_gc_gap32"])
    for k, gc in enumerate(grads):
        want = g["%s_gc64_%d" % (tag, k)]
        assert gc.dtype == dt and tuple(gc.shape) == want.shape
        err = np.abs(gc.double().cpu().numpy() - want).max()
        if precision == 64:
            assert err <= 1e-12 * max(1.0, np.abs(want).max()), (k, err)
        else:
            assert err <= gap, (k, err, gap)


DOT_CASES = [   # size, height, nbands, n: even / odd sides, side > 96, nbands 2-4 and 16, height 2, N > 1
    (64, 4, 3, 1), (75, 4, 2, 1), (130, 5, 2, 1), (33, 3, 4, 1), (32, 3, 16, 1), (32, 2, 2, 2), (50, 3, 2, 3)]


@pytest.mark.parametrize("size,height,nbands,n", DOT_CASES)
def test_build_adjoint_identity(pkg, dev, size, height, nbands, n):
    """<build(x), w> == <x, build^T w> at precision 64, and (N > 1) each image's gradient is its own."""
    pyr = _pyr(height, nbands, dev, 64)
    x = _rand((n, 1, size, size), size, dev).requires_grad_()
    flat = _flatten(pyr.build(x))
    w = [_rand(c.shape, 100 + k, dev) for k, c in enumerate(flat)]
    (gx,) = torch.autograd.grad(flat, x, grad_outputs=w)
    lhs, rhs = _dot(flat, w), _dot([x], [gx])
    assert abs(lhs - rhs) <= 1e-12 * _norm([x]) * _norm([gx]), (lhs, rhs)
    for k in range(n if n > 1 else 0):
        xk = x[k:k + 1].detach().clone().requires_grad_()
        fk = _flatten(pyr.build(xk))
        (gk,) = torch.autograd.grad(fk, xk, grad_outputs=[t[k:k + 1] for t in w])
        assert torch.equal(gk[0], gx[k]), k


@pytest.mark.parametrize("size,height,nbands,n", DOT_CASES)
def test_reconstruct_adjoint_identity(pkg, dev, size, height, nbands, n):
    """<reconstruct(c), y> == <c, reconstruct^T y> at precision 64, and (N > 1) each image's gradients are its own."""
    pyr = _pyr(height, nbands, dev, 64)
    shapes = cases.shapes(size, height, nbands, n)
    flat = [_rand(s, 200 + k, dev).requires_grad_() for k, s in enumerate(shapes)]
    out = pyr.reconstruct(_nest(flat, height, nbands))
    y = _rand(out.shape, size + 1, dev)
    grads = torch.autograd.grad(out, flat, grad_outputs=y)
    lhs, rhs = _dot([out], [y]), _dot(flat, grads)
    assert abs(lhs - rhs) <= 1e-12 * _norm(flat) * _norm(grads), (lhs, rhs)
    for k in range(n if n > 1 else 0):
        fk = [c[k:k + 1].detach().clone().requires_grad_() for c in flat]
        gk = torch.autograd.grad(pyr.reconstruct(_nest(fk, height, nbands)), fk, grad_outputs=y[k:k + 1])
        for a, b in zip(gk, grads):
            assert torch.equal(a[0], b[k]), k


def test_gradcheck_and_gradgradcheck(pkg, dev):
    pyr = _pyr(3, 2, dev, 64)
    x = _rand((1, 1, 32, 32), 1, dev).requires_grad_()
    build = lambda t: tuple(_flatten(pyr.build(t)))
    assert torch.autograd.gradcheck(build, (x,), fast_mode=True)
    assert torch.autograd.gradgradcheck(build, (x,), fast_mode=True)
    flat = [_rand(s, 10 + k, dev).requires_grad_() for k, s in enumerate(cases.shapes(32, 3, 2, 1))]
    recon = lambda *c: pyr.reconstruct(_nest(list(c), 3, 2))
    assert torch.autograd.gradcheck(recon, tuple(flat), fast_mode=True)
    assert torch.autograd.gradgradcheck(recon, tuple(flat), fast_mode=True)


@pytest.mark.parametrize("precision", [32, 64])
def test_forward_unchanged_on_the_grad_path(pkg, dev, precision):
    dt = torch.float32 if precision == 32 else torch.float64
    pyr = _pyr(4, 2, dev, precision)
    x = _rand((2, 1, 75, 75), 3, dev, dt)
    plain = _flatten(pyr.build(x))
    assert all(c.grad_fn is None for c in plain)
    xg = x.clone().requires_grad_()
    tracked = _flatten(pyr.build(xg))
    assert all(c.grad_fn is not None for c in tracked)
    assert all(torch.equal(a, b) for a, b in zip(plain, tracked))
    with torch.no_grad():
        assert all(c.grad_fn is None for c in _flatten(pyr.build(xg)))
    rec = pyr.reconstruct(_nest(plain, 4, 2))
    assert rec.grad_fn is None
    rec_g = pyr.reconstruct(_nest(tracked, 4, 2))
    assert rec_g.grad_fn is not None and torch.equal(rec, rec_g)
    with torch.no_grad():
        assert pyr.reconstruct(_nest(tracked, 4, 2)).grad_fn is None


def test_missing_expanded_and_non_contiguous_upstream_gradients(pkg, dev):
    pyr = _pyr(4, 2, dev, 64)
    x = _rand((2, 1, 64, 64), 4, dev).requires_grad_()
    flat = _flatten(pyr.build(x))
    w1 = _rand(flat[1].shape, 5, dev)
    (one,) = torch.autograd.grad((flat[1] * w1).sum(), x, retain_graph=True)      # every other gradient missing
    full = [torch.zeros_like(c) for c in flat]
    full[1] = w1
    (want,) = torch.autograd.grad(flat, x, grad_outputs=full, retain_graph=True)
    assert torch.equal(one, want)
    (expanded,) = torch.autograd.grad(flat[0].sum() + flat[-1].sum(), x, retain_graph=True)   # stride-0 upstream gradients
    ones = [torch.zeros_like(c) for c in flat]
    ones[0], ones[-1] = torch.ones_like(flat[0]), torch.ones_like(flat[-1])
    (want,) = torch.autograd.grad(flat, x, grad_outputs=ones, retain_graph=True)
    assert torch.equal(expanded, want)
    w = [_rand(c.shape, 20 + k, dev) for k, c in enumerate(flat)]
    strided = [t.transpose(1, 2).contiguous().transpose(1, 2) for t in w]        # same values, non-contiguous
    assert not strided[0].is_contiguous()
    (a,) = torch.autograd.grad(flat, x, grad_outputs=w, retain_graph=True)
    (b,) = torch.autograd.grad(flat, x, grad_outputs=strided)
    assert torch.equal(a, b)
    # reconstruct: a non-contiguous image gradient, and coefficients only partly requiring grad
    shapes = cases.shapes(64, 4, 2, 2)
    coeffs = [_rand(s, 30 + k, dev) for k, s in enumerate(shapes)]
    y = _rand((2, 64, 64), 6, dev)
    req = [c.clone().requires_grad_() for c in coeffs]
    all_g = torch.autograd.grad(pyr.reconstruct(_nest(req, 4, 2)), req, grad_outputs=y)
    part = [c.clone().requires_grad_(k % 2 == 0) for k, c in enumerate(coeffs)]
    out = pyr.reconstruct(_nest(part, 4, 2))
    y_strided = y.transpose(1, 2).contiguous().transpose(1, 2)
    some = torch.autograd.grad(out, [c for c in part if c.requires_grad], grad_outputs=y_strided)
    assert all(torch.equal(s, a) for s, a in zip(some, all_g[::2]))
    part[0].grad = None
    pyr.reconstruct(_nest(part, 4, 2)).backward(y)
    assert torch.equal(part[0].grad, all_g[0]) and all(c.grad is None for c in part[1::2])


def test_backward_after_the_pyramid_was_used_at_another_size(pkg, dev):
    """_get replaces the native handle when the size changes: the backward re-resolves it by size."""
    x = _rand((1, 1, 64, 64), 7, dev).requires_grad_()
    fresh = _pyr(4, 2, dev, 64)
    w = [_rand(c.shape, 40 + k, dev) for k, c in enumerate(_flatten(fresh.build(x.detach())))]
    (want,) = torch.autograd.grad(_flatten(fresh.build(x)), x, grad_outputs=w)
    pyr = _pyr(4, 2, dev, 64)
    flat = _flatten(pyr.build(x))
    other = pyr.build(_rand((2, 1, 75, 75), 8, dev).requires_grad_())      # replaces the 64 handle
    (got,) = torch.autograd.grad(flat, x, grad_outputs=w)
    assert torch.equal(got, want)
    coeffs = [c.detach().clone().requires_grad_() for c in _flatten(other)]
    out = pyr.reconstruct(_nest(coeffs, 4, 2))
    pyr.build(x.detach())                                                  # back to 64
    y = _rand(out.shape, 9, dev)
    got = torch.autograd.grad(out, coeffs, grad_outputs=y)
    fresh75 = _pyr(4, 2, dev, 64)
    ref = [c.detach().clone().requires_grad_() for c in coeffs]
    want = torch.autograd.grad(fresh75.reconstruct(_nest(ref, 4, 2)), ref, grad_outputs=y)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("precision", [32, 64])
def test_backward_is_deterministic(pkg, dev, precision):
    dt = torch.float32 if precision == 32 else torch.float64
    pyr = _pyr(5, 2, dev, precision)
    x = _rand((2, 1, 130, 130), 11, dev, dt).requires_grad_()
    flat = _flatten(pyr.build(x))
    w = [_rand(c.shape, 50 + k, dev, dt) for k, c in enumerate(flat)]
    (a,) = torch.autograd.grad(flat, x, grad_outputs=w, retain_graph=True)
    (b,) = torch.autograd.grad(flat, x, grad_outputs=w)
    assert torch.equal(a, b)
    coeffs = [t.clone().requires_grad_() for t in w]
    out = pyr.reconstruct(_nest(coeffs, 5, 2))
    y = _rand(out.shape, 12, dev, dt)
    ga = torch.autograd.grad(out, coeffs, grad_outputs=y, retain_graph=True)
    gb = torch.autograd.grad(out, coeffs, grad_outputs=y)
    assert all(torch.equal(p, q) for p, q in zip(ga, gb))


def test_adjoint_c_abi_errors(pkg, dev):
    from mimamo_net_amd import _lib
    L = _lib.lib()
    pyr = _pyr(4, 2, dev, 64)
    h = pyr._get(96)
    coeff = [torch.zeros(s, dtype=torch.float64, device=dev) for s in cases.shapes(96, 4, 2, 2)]
    img = torch.zeros(2, 96, 96, dtype=torch.float64, device=dev)
    ws_bytes = L.mm_scfpyr_workspace_bytes(h, 2)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    vp = ctypes.c_void_p
    s = _lib.current_stream()
    ptrs = (vp * len(coeff))(*[c.data_ptr() for c in coeff])
    holes = (vp * len(coeff))(*[c.data_ptr() for c in coeff])
    holes[3] = None
    im, w = vp(img.data_ptr()), vp(ws.data_ptr())
    for call in (lambda hh, pp, prec, n, o, wp, wb: L.mm_scfpyr_build_adjoint(hh, pp, prec, n, o, wp, wb, s),
                 lambda hh, pp, prec, n, o, wp, wb: L.mm_scfpyr_reconstruct_adjoint(hh, o, prec, n, pp, wp, wb, s)):
        assert call(h, ptrs, 64, 2, im, w, ws_bytes - 1) == _lib.MM_ERR_WORKSPACE
        assert call(None, ptrs, 64, 2, im, w, ws_bytes) == _lib.MM_ERR_INVALID_ARG
        assert call(h, None, 64, 2, im, w, ws_bytes) == _lib.MM_ERR_INVALID_ARG
        assert call(h, ptrs, 64, 2, None, w, ws_bytes) == _lib.MM_ERR_INVALID_ARG
        assert call(h, ptrs, 64, 2, im, None, ws_bytes) == _lib.MM_ERR_INVALID_ARG
        assert call(h, ptrs, 16, 2, im, w, ws_bytes) == _lib.MM_ERR_INVALID_ARG
        assert call(h, ptrs, 64, -1, im, w, ws_bytes) == _lib.MM_ERR_INVALID_ARG
        assert call(h, holes, 64, 2, im, w, ws_bytes) == _lib.MM_ERR_INVALID_ARG
        assert call(h, None, 64, 0, None, None, 0) == _lib.MM_OK                   # n == 0: no-op
        assert call(h, ptrs, 64, 2, im, w, ws_bytes) == _lib.MM_OK
    torch.cuda.synchronize()
    assert img.abs().max().item() == 0.0 and all(c.abs().max().item() == 0.0 for c in coeff)   # zero in, zero out


def test_general_build_pyramid_is_differentiable(pkg, dev):
    """Phase_Difference_Extractor.build_pyramid on a configuration the fused kernels reject: its mirror / stack / crop are torch
    ops around SCFpyr_PyTorch.build, so the gradient to im_batch passes the adjoint identity (fp32)."""
    from mimamo_net_amd.phase_difference_extractor import Phase_Difference_Extractor
    pde = Phase_Difference_Extractor(height=4, nbands=4, scale_factor=2, extract_level=[1, 2])
    assert not pde._fused(32, True)
    x = _rand((2, 3, 32, 32), 13, dev, torch.float32).requires_grad_()
    outs = pde.build_pyramid(x, symmetry=True)
    w = [_rand(o.shape, 60 + k, dev, torch.float32) for k, o in enumerate(outs)]
    (gx,) = torch.autograd.grad(outs, x, grad_outputs=w)
    lhs, rhs = _dot(outs, w), _dot([x], [gx])
    assert abs(lhs - rhs) <= 1e-5 * _norm([x]) * _norm([gx]), (lhs, rhs)
    with torch.no_grad():
        plain = pde.build_pyramid(x, symmetry=True)
    assert all(torch.equal(a, b) for a, b in zip(plain, outs))


def test_fused_build_pyramid_stays_inference_only(pkg, dev):
    from mimamo_net_amd.phase_difference_extractor import Phase_Difference_Extractor
    pde = Phase_Difference_Extractor(height=4, nbands=2, scale_factor=2, extract_level=1)
    x = _rand((1, 3, 48, 48), 14, dev, torch.float32).requires_grad_()
    out = pde.build_pyramid(x)
    assert pde._fused(48, True) and out.grad_fn is None
