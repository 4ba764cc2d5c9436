"""SCFpyr_PyTorch.reconstruct without a GPU: the host-side reconstruct multipliers (mm_scfpyr_host_recon_table), applied with
numpy's FFTs in the convention include/mimamo_hip.h documents, reproduce the real reference's precision=64 reconstruction
(tests/golden/scfpyr_reconstruct.npz, make_golden_reconstruct.py) on every fixture case.  The inputs are regenerated
(scfpyr_recon_cases.py); image cases take the pyramid from the build's host tables, pinned to the reference's build by G8."""
import ctypes

import numpy as np
import pytest

import scfpyr_recon_cases as cases


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


def _host_build(L, height, nbands):
    """The library's build on the host: its per-output tables applied with numpy's FFT (test_capi_cpu.py, G8)."""
    def build(x):
        size = x.shape[-1]
        F = np.fft.fft2(x[:, 0])
        flat = []
        for i in range(2 + (height - 2) * nbands):
            T, is_complex = _table(L.mm_scfpyr_host_table, size, height, nbands, i)
            m, fa = T.shape[0], _signed(T.shape[0], size)
            o = np.fft.ifft2(F[:, fa][:, :, fa] * T) * (m * m)
            flat.append(np.stack([o.real, o.imag], -1) if is_complex else o.real)
        return flat
    return build


@pytest.mark.parametrize("tag", sorted(cases.CASES))
def test_recon_tables_reproduce_reference_reconstruct(L, golden, tag):
    g = golden("scfpyr_reconstruct")
    size, height, nbands, n = cases.CASES[tag][:4]
    flat = cases.inputs(tag, g, _host_build(L, height, nbands))
    S = np.zeros((n, size, size), dtype=np.complex128)
    for i, c in enumerate(flat):
        R, is_complex = _table(L.mm_scfpyr_host_recon_table, size, height, nbands, i)
        assert is_complex == (0 < i < len(flat) - 1)
        if is_complex:
            c = c[..., 0] + 1j * c[..., 1]
        m = R.shape[0]
        assert c.shape == (n, m, m)
        fa = _signed(m, size)
        S[:, fa[:, None], fa[None, :]] += np.fft.fft2(c) * R
    got = (np.fft.ifft2(S) * (size * size)).real             # unnormalised inverse: 1/size^2 sits in the tables
    want = g[tag + "_out64"]
    err = np.abs(got - want).max()
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), err


def test_recon_tables_match_build_tables_in_shape(L):
    """Same order, sides and kinds as the build's outputs, so one handle's output_info serves both directions."""
    side, cp, rside, rcp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for size, height, nbands in ((96, 4, 2), (75, 4, 3), (130, 5, 2)):
        for i in range(2 + (height - 2) * nbands):
            assert L.mm_scfpyr_host_table(size, height, nbands, 2, i, None, ctypes.byref(side), ctypes.byref(cp)) == 0
            assert L.mm_scfpyr_host_recon_table(size, height, nbands, 2, i, None, ctypes.byref(rside), ctypes.byref(rcp)) == 0
            assert (side.value, cp.value) == (rside.value, rcp.value)


def test_recon_table_config_errors(L):
    side, cp = ctypes.c_int(), ctypes.c_int()
    q = lambda size, height, nbands, index=0: L.mm_scfpyr_host_recon_table(size, height, nbands, 2, index, None,
                                                                             ctypes.byref(side), ctypes.byref(cp))
    assert q(96, 5, 2) == -2          # image too small (SCFpyr_PyTorch.py:90-91)
    assert q(96, 4, 1) == -3          # nbands < 2: unsupported
    assert q(96, 4, 17) == -3         # nbands > 16
    assert q(1026, 4, 2) == -3        # side above 1024
    assert q(96, 4, 2, 6) == -1       # 2 + 2 * 2 = 6 outputs: index 6 is out of range
    assert q(96, 4, 2, -1) == -1
    assert q(96, 4, 2, 5) == 0 and side.value == 24 and cp.value == 0
    assert L.mm_scfpyr_host_recon_table(96, 4, 2, 2, 0, None, None, ctypes.byref(cp)) == -1
