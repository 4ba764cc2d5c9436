"""GPU: SCFpyr_PyTorch.reconstruct (csrc/scfpyr.hip, mm_scfpyr_reconstruct) vs the real reference's reconstruction
(tests/golden/scfpyr_reconstruct.npz), the library's own build -> reconstruct round trip, determinism and the error paths.
The fixture's inputs are regenerated (scfpyr_recon_cases.py); image cases take the pyramid from the library's precision-64
build, pinned to the reference's build by G8."""
import ctypes

import numpy as np
import pytest
import torch

import scfpyr_recon_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _flatten(coeff):
    return [coeff[0]] + [b for level in coeff[1:-1] for b in level] + [coeff[-1]]


def _case(g, tag, dev):
    size, height, nbands, n = cases.CASES[tag][:4]
    pyr = _pyr(height, nbands, dev, 64)
    build = lambda x: [c.cpu().numpy() for c in _flatten(pyr.build(torch.from_numpy(x).to(dev)))]
    return size, height, nbands, n, cases.inputs(tag, g, build)


def _nest(flat, height, nbands):
    return [flat[0]] + [list(flat[1 + l * nbands:1 + (l + 1) * nbands]) for l in range(height - 2)] + [flat[-1]]


def _to(flat, dev, dt):
    return [torch.from_numpy(c).to(dev, dt) for c in flat]


def _pyr(height, nbands, dev, precision):
    from mimamo_net_amd.scfpyr import SCFpyr_PyTorch
    return SCFpyr_PyTorch(height=height, nbands=nbands, scale_factor=2, device=dev, precision=precision)


@pytest.mark.parametrize("tag", sorted(cases.CASES))
@pytest.mark.parametrize("precision", [32, 64])
def test_reconstruct_golden(pkg, golden, dev, tag, precision):
    g = golden("scfpyr_reconstruct")
    size, height, nbands, n, flat = _case(g, tag, dev)
    dt = torch.float32 if precision == 32 else torch.float64
    got = _pyr(height, nbands, dev, precision).reconstruct(_nest(_to(flat, dev, dt), height, nbands))
    assert got.dtype == dt and got.device == dev and tuple(got.shape) == (n, size, size)
    want = g[tag + "_out64"]
    err = np.abs(got.double().cpu().numpy() - want).max()
    if precision == 64:
        assert err <= 1e-12 * max(1.0, np.abs(want).max()), err
    else:   # float64 inside: no worse than the reference's own fp32 reconstruction of the same coefficients
        assert err <= float(g[tag + "_gap32"]), (err, float(g[tag + "_gap32"]))


@pytest.mark.parametrize("tag", cases.IMAGE_CASES)
def test_build_then_reconstruct_round_trip(pkg, golden, dev, tag):
    """The library's build followed by its reconstruct is as close to the image as the reference's own round trip (the
    residual is the raised-cosine lookup-table interpolation, not arithmetic)."""
    g = golden("scfpyr_reconstruct")
    size, height, nbands, n = cases.CASES[tag][:4]
    x = cases.image(tag)
    pyr = _pyr(height, nbands, dev, 64)
    rec = pyr.reconstruct(pyr.build(torch.from_numpy(x).to(dev)))
    x = x[:, 0]
    err = np.abs(rec.cpu().numpy() - x).max()
    assert abs(err - float(g[tag + "_rt_err"])) <= 1e-9, (err, float(g[tag + "_rt_err"]))


@pytest.mark.parametrize("size,height,nbands,precision", [(75, 4, 2, 64), (96, 4, 3, 32), (130, 5, 2, 32)])
def test_reconstruct_is_deterministic_and_batch_independent(pkg, dev, size, height, nbands, precision):
    from mimamo_net_amd import weights
    dt = torch.float32 if precision == 32 else torch.float64
    x = torch.from_numpy(weights.det_uniform("scf.recon.det", (3, 1, size, size), 0.0, 1.0, size)).to(dev, dt)
    pyr = _pyr(height, nbands, dev, precision)
    coeff = pyr.build(x)
    a = pyr.reconstruct(coeff)
    b = pyr.reconstruct(coeff)
    assert torch.equal(a, b)
    for k in range(3):
        one = [coeff[0][k:k + 1]] + [[t[k:k + 1] for t in lvl] for lvl in coeff[1:-1]] + [coeff[-1][k:k + 1]]
        assert torch.equal(pyr.reconstruct(one)[0], a[k]), k


def test_reconstruct_accepts_non_contiguous_coefficients(pkg, golden, dev):
    g = golden("scfpyr_reconstruct")
    size, height, nbands, n, flat = _case(g, "h", dev)
    pyr = _pyr(height, nbands, dev, 64)
    want = pyr.reconstruct(_nest(_to(flat, dev, torch.float64), height, nbands))
    strided = []
    for c in flat:
        t = torch.from_numpy(c).to(dev)
        big = torch.zeros((c.shape[0], c.shape[1], 2 * c.shape[2]) + c.shape[3:], dtype=torch.float64, device=dev)
        big[:, :, 1::2] = t
        strided.append(big[:, :, 1::2])
        assert not strided[-1].is_contiguous()
    got = pyr.reconstruct(_nest(strided, height, nbands))
    assert torch.equal(got, want)


def test_reconstruct_height_2_any_batch_size(pkg, dev):
    """With height 2 the list is [hi, lo]; the reference only accepts N == nbands there (SCFpyr_PyTorch.py:216 compares
    nbands with len(lo)).  Deliberate difference: any N."""
    from mimamo_net_amd import weights
    x = weights.det_uniform("scf.recon.h2", (3, 1, 32, 32), 0.0, 1.0, 1).astype(np.float64)
    pyr = _pyr(2, 2, dev, 64)
    coeff = pyr.build(torch.from_numpy(x).to(dev))
    assert len(coeff) == 2
    rec = pyr.reconstruct(coeff)
    assert tuple(rec.shape) == (3, 32, 32)
    assert np.abs(rec.cpu().numpy() - x[:, 0]).max() < 2e-5


def test_reconstruct_errors(pkg, dev):
    pyr = _pyr(4, 2, dev, 32)
    coeff = pyr.build(torch.zeros(2, 1, 96, 96, device=dev))
    with pytest.raises(Exception, match="Unmatched number of orientations"):
        pyr.reconstruct([coeff[0], coeff[1][:1], coeff[2], coeff[3]])
    with pytest.raises(Exception, match="Unmatched number of orientations"):
        _pyr(4, 3, dev, 32).reconstruct(coeff)
    with pytest.raises(ValueError):
        pyr.reconstruct(coeff[:-1])                                            # levels
    with pytest.raises(ValueError):
        pyr.reconstruct([coeff[0], coeff[1], coeff[2], coeff[3][:, :-1]])     # lo shape
    with pytest.raises(ValueError):
        pyr.reconstruct([coeff[0], [coeff[1][0][..., 0], coeff[1][1]], coeff[2], coeff[3]])   # band without re/im
    with pytest.raises(ValueError):
        pyr.reconstruct([coeff[0][:1], coeff[1], coeff[2], coeff[3]])         # batch sizes disagree
    with pytest.raises(ValueError):
        pyr.reconstruct([coeff[0][:, :, :-1], coeff[1], coeff[2], coeff[3]])  # hi not square
    with pytest.raises(AssertionError, match="Image batch must be torch.float64"):
        _pyr(4, 2, dev, 64).reconstruct(coeff)                               # dtype
    with pytest.raises(AssertionError, match="Devices invalid"):
        pyr.reconstruct([coeff[0].cpu()] + coeff[1:])                         # CPU tensors: no CPU path
    empty = pyr.reconstruct(pyr.build(torch.zeros(0, 1, 96, 96, device=dev)))
    assert tuple(empty.shape) == (0, 96, 96)


def test_reconstruct_c_abi_errors(pkg, dev):
    from mimamo_net_amd import _lib
    L = _lib.lib()
    pyr = _pyr(4, 2, dev, 64)
    coeff = pyr.build(torch.zeros(2, 1, 96, 96, device=dev, dtype=torch.float64))
    flat = [coeff[0]] + coeff[1] + coeff[2] + [coeff[3]]
    h = pyr._get(96)
    out = torch.empty(2, 96, 96, dtype=torch.float64, device=dev)
    ws_bytes = L.mm_scfpyr_workspace_bytes(h, 2)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    ptrs = (ctypes.c_void_p * len(flat))(*[c.data_ptr() for c in flat])
    vp = ctypes.c_void_p
    s = _lib.current_stream()
    call = lambda hh, pp, prec, n, o, w, wb: L.mm_scfpyr_reconstruct(hh, pp, prec, n, o, w, wb, s)
    assert call(h, ptrs, 64, 2, vp(out.data_ptr()), vp(ws.data_ptr()), ws_bytes - 1) == _lib.MM_ERR_WORKSPACE
    assert call(None, ptrs, 64, 2, vp(out.data_ptr()), vp(ws.data_ptr()), ws_bytes) == _lib.MM_ERR_INVALID_ARG
    assert call(h, None, 64, 2, vp(out.data_ptr()), vp(ws.data_ptr()), ws_bytes) == _lib.MM_ERR_INVALID_ARG
    assert call(h, ptrs, 64, 2, None, vp(ws.data_ptr()), ws_bytes) == _lib.MM_ERR_INVALID_ARG
    assert call(h, ptrs, 64, 2, vp(out.data_ptr()), None, ws_bytes) == _lib.MM_ERR_INVALID_ARG
    assert call(h, ptrs, 16, 2, vp(out.data_ptr()), vp(ws.data_ptr()), ws_bytes) == _lib.MM_ERR_INVALID_ARG
    assert call(h, ptrs, 64, -1, vp(out.data_ptr()), vp(ws.data_ptr()), ws_bytes) == _lib.MM_ERR_INVALID_ARG
    holes = (ctypes.c_void_p * len(flat))(*[c.data_ptr() for c in flat])
    holes[3] = None
    assert call(h, holes, 64, 2, vp(out.data_ptr()), vp(ws.data_ptr()), ws_bytes) == _lib.MM_ERR_INVALID_ARG
    assert call(h, None, 64, 0, None, None, 0) == _lib.MM_OK                   # n == 0: no-op
    assert call(h, ptrs, 64, 2, vp(out.data_ptr()), vp(ws.data_ptr()), ws_bytes) == _lib.MM_OK
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0.0                                       # the zero image's pyramid


def test_reconstruct_leaves_default_dtype_alone(pkg, dev):
    before = torch.get_default_dtype()
    pyr = _pyr(3, 2, dev, 64)
    pyr.reconstruct(pyr.build(torch.zeros(1, 1, 32, 32, device=dev, dtype=torch.float64)))
    assert torch.get_default_dtype() == before
