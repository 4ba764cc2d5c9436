"""SCFpyr_PyTorch gradients without a GPU: the existing host tables (mm_scfpyr_host_table, mm_scfpyr_host_recon_table),
conjugated and applied with numpy's FFTs in the adjoint form include/mimamo_hip.h documents for mm_scfpyr_build_adjoint /
mm_scfpyr_reconstruct_adjoint, reproduce the real reference's torch-autograd gradients (tests/golden/scfpyr_grad.npz,
make_golden_scfpyr_grad.py) on every fixture case.  This pins the convention the kernels implement.  The cotangents are
regenerated (scfpyr_grad_cases.py)."""
import ctypes

import numpy as np
import pytest

import scfpyr_grad_cases as cases


@pytest.fixture(scope="module")
def L(pkg):
    from mimamo_net_amd import build, _lib
    build.build_library()
    return _lib.lib()


def _table(fn, size, height, nbands, index):
    side, cp = ctypes.c_int(), ctypes.c_int()
    assert fn(size, height, nbands, 2, index, None, ctypes.byref(side), ctypes.byref(cp)) == 0
    t = np.zeros((side.value, side.value, 2))
    assert fn(size, height, nbands, 2, index, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(side),
              ctypes.byref(cp)) == 0
    return t[..., 0] + 1j * t[..., 1], bool(cp.value)


def _signed(m, size):
    k = np.arange(m)
    return np.where(k < (m + 1) // 2, k, k - m) % size      # signed frequency (odd m: one more non-negative) modulo the image side


def _close(got, want):
    err = np.abs(got - want).max()
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), err


@pytest.mark.parametrize("tag", sorted(cases.CASES))
def test_conjugated_build_tables_reproduce_reference_build_gradient(L, golden, tag):
    g = golden("scfpyr_grad")
    cases.check_cfg(g, tag)
    size, height, nbands, n = cases.CASES[tag][:4]
    S = np.zeros((n, size, size), dtype=np.complex128)
    for i, w in enumerate(cases.coeff_cotangents(tag)):
        T, is_complex = _table(L.mm_scfpyr_host_table, size, height, nbands, i)
        if is_complex:
            w = w[..., 0] + 1j * w[..., 1]
        m = T.shape[0]
        assert w.shape == (n, m, m)
        fa = _signed(m, size)
        S[:, fa[:, None], fa[None, :]] += np.conj(T) * np.fft.fft2(w)
    got = (np.fft.ifft2(S) * (size * size)).real             # unnormalised inverse
    want = g[tag + "_gx64"]
    assert want.shape == (n, 1, size, size)
    _close(got, want[:, 0])


@pytest.mark.parametrize("tag", cases.RECON_CASES)
def test_conjugated_recon_tables_reproduce_reference_reconstruct_gradient(L, golden, tag):
    g = golden("scfpyr_grad")
    cases.check_cfg(g, tag)
    size, height, nbands, n = cases.CASES[tag][:4]
    Y = np.fft.fft2(cases.image_cotangent(tag))
    shapes = cases.shapes(size, height, nbands, n)
    for i, shp in enumerate(shapes):
        R, is_complex = _table(L.mm_scfpyr_host_recon_table, size, height, nbands, i)
        m = R.shape[0]
        fa = _signed(m, size)
        c = np.fft.ifft2(np.conj(R) * Y[:, fa[:, None], fa[None, :]]) * (m * m)
        got = np.stack([c.real, c.imag], -1) if is_complex else c.real
        want = g["%s_gc64_%d" % (tag, i)]
        assert got.shape == want.shape == shp
        _close(got, want)
    assert "%s_gc64_%d" % (tag, len(shapes)) not in g


def test_library_exports_the_adjoints(L):
    from mimamo_net_amd import _lib
    for name in ("mm_scfpyr_build_adjoint", "mm_scfpyr_reconstruct_adjoint"):
        assert name in _lib.SIGNATURES
        fn = getattr(L, name)
        assert fn.restype == ctypes.c_int and len(fn.argtypes) == 8
