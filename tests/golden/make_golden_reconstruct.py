"""Freeze SCFpyr_PyTorch.reconstruct of the REAL reference (imported via ref_shim) as a data fixture.
Run once in the build container:  python tests/golden/make_golden_reconstruct.py

  scfpyr_reconstruct.npz  for every case: the reference's precision=64 reconstruction, and the max difference of its
                    precision=32 reconstruction (same coefficients cast to float32) from it; for image cases also the
                    reference's own round-trip error max |reconstruct(build(x)) - x| at precision=64.

The input coefficients are not stored: like make_golden.py, only the generator arguments (CASES, mirrored by the tests)
and the reference's outputs are.  The tests regenerate the inputs from the repo's own closed-form generator
(mimamo-net_amd/weights.py det_uniform): image cases feed the reference's build of the image -- which the tests reproduce
with the library's build, pinned to the reference by G8 -- case h edits such a pyramid (the rotation angles are stored),
case i has det_uniform values in every coefficient.

Cases a-f are G8's grids and images (make_golden.py SCF_FULL_CASES), g is a side above 96, h an edited pyramid, i
arbitrary values in every coefficient, j height 2 with N == nbands (the only N the reference accepts there).

On top of ref_shim's five shims this adds, in memory, a sixth:

  6. torch.fft(x, signal_ndim=2)     (old callable API, SCFpyr_PyTorch.py:257): on current torch `torch.fft` is a
                                     module; its class is swapped for a ModuleType subclass whose __call__ maps
                                     [...,2] to view_as_real(fft2(view_as_complex(x))).  The module's functions stay.

Fixtures are data only; no reference source is stored.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_shim  # noqa: E402
import mimamo_net_amd  # noqa: E402,F401
from mimamo_net_amd import weights  # noqa: E402


class _CallableFFT(types.ModuleType):
    def __call__(self, x, signal_ndim=2, normalized=False):
        assert signal_ndim == 2 and not normalized
        return torch.view_as_real(torch.fft.fft2(torch.view_as_complex(x.contiguous())))


def _install_fft_shim():
    if not callable(torch.fft):  # shim 6
        torch.fft.__class__ = _CallableFFT


CASES = [
    # tag, size, height, nbands, n_images, det_uniform key, seed, kind
    ("a", 96, 4, 2, 1, "scf.a", 8, "image"),
    ("b", 32, 3, 4, 2, "scf.b", 9, "image"),
    ("c", 32, 3, 3, 1, "scf.c", 10, "image"),
    ("d", 50, 3, 2, 1, "scf.d", 11, "image"),
    ("e", 75, 4, 2, 1, "scf.e", 12, "image"),
    ("f", 84, 4, 2, 1, "scf.f", 13, "image"),
    ("g", 130, 5, 2, 1, "scf.g", 14, "image"),       # side above 96: the transforms' scratch path
    ("h", 75, 4, 2, 1, "scf.e", 12, "edited"),       # case e's pyramid with every band rotated, hi halved, lo shifted
    ("i", 50, 3, 3, 2, "scf.recon.i", 15, "random"),  # arbitrary values in every coefficient
    ("j", 32, 2, 2, 2, "scf.j", 16, "image"),        # height 2: [hi, lo]; the reference needs N == nbands here
]


def shapes(size, height, nbands, n):
    out = [(n, size, size)]
    s = size
    for _ in range(height - 2):
        out += [(n, s, s, 2)] * nbands
        s = int(np.ceil((s - 0.5) / 2))
    return out + [(n, s, s)]


def random_coefficients(key, seed, size, height, nbands, n):
    return [weights.det_uniform("%s.%d" % (key, k), shp, -1.0, 1.0, seed).astype(np.float64)
            for k, shp in enumerate(shapes(size, height, nbands, n))]


def edit(flat, theta):
    """bands times e^{i theta_k} (k = level-major band index), hi-pass residual halved, low-pass residual + 0.1"""
    flat = list(flat)
    for k, t in enumerate(theta):
        c = flat[1 + k]
        z = (c[..., 0] + 1j * c[..., 1]) * np.exp(1j * t)
        flat[1 + k] = np.stack([z.real, z.imag], -1)
    flat[0] = flat[0] * 0.5
    flat[-1] = flat[-1] + 0.1
    return flat


def flatten(coeff):
    return [coeff[0]] + [b for level in coeff[1:-1] for b in level] + [coeff[-1]]


def nest(flat, height, nbands):
    out = [flat[0]]
    for l in range(height - 2):
        out.append(flat[1 + l * nbands:1 + (l + 1) * nbands])
    out.append(flat[-1])
    return out


def reconstruct(ref, flat, height, nbands, precision):
    dt = torch.float64 if precision == 64 else torch.float32
    pyr = ref.SCFpyr_PyTorch(height=height, nbands=nbands, scale_factor=2, device=torch.device("cpu"), precision=precision)
    out = pyr.reconstruct(nest([torch.from_numpy(c).to(dt) for c in flat], height, nbands))
    torch.set_default_dtype(torch.float32)
    return out.numpy()


def main():
    ref = ref_shim.load()
    _install_fft_shim()
    out = {}
    for tag, size, height, nbands, n, key, seed, kind in CASES:
        x = None
        if kind == "random":
            flat = random_coefficients(key, seed, size, height, nbands, n)
        else:
            x = weights.det_uniform(key, (n, 1, size, size), 0.0, 1.0, seed).astype(np.float64)
            pyr = ref.SCFpyr_PyTorch(height=height, nbands=nbands, scale_factor=2, device=torch.device("cpu"), precision=64)
            flat = [c.numpy().copy() for c in flatten(pyr.build(torch.from_numpy(x)))]
            torch.set_default_dtype(torch.float32)
        if kind == "edited":
            theta = np.linspace(-2.5, 2.9, (height - 2) * nbands)
            flat = edit(flat, theta)
            out["%s_theta" % tag] = theta
            x = None
        assert [c.shape for c in flat] == shapes(size, height, nbands, n)
        o64 = reconstruct(ref, flat, height, nbands, 64)
        o32 = reconstruct(ref, flat, height, nbands, 32)
        out["%s_cfg" % tag] = np.array([size, height, nbands, n, len(flat)], dtype=np.int64)
        out["%s_out64" % tag] = o64.astype(np.float64)
        out["%s_gap32" % tag] = np.float64(np.abs(o32.astype(np.float64) - o64).max())
        msg = "fp32 gap %.2e" % out["%s_gap32" % tag]
        if x is not None:
            out["%s_rt_err" % tag] = np.float64(np.abs(o64 - x[:, 0]).max())
            msg += ", round trip %.2e" % out["%s_rt_err" % tag]
        print(tag, size, height, nbands, n, kind, o64.shape, msg)
    np.savez_compressed(os.path.join(HERE, "scfpyr_reconstruct.npz"), **out)


if __name__ == "__main__":
    main()
