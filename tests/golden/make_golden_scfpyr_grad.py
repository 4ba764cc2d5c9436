"""Freeze torch-autograd gradients of the REAL reference's SCFpyr_PyTorch (imported via ref_shim) as a data fixture.
Run once in the build container:  python tests/golden/make_golden_scfpyr_grad.py

  scfpyr_grad.npz   for every case (tests/scfpyr_grad_cases.py):
                      <tag>_gx64       d<build(x), w>/dx at precision=64, [n, 1, size, size]: the build's vector-Jacobian
                                       product with the case's coefficient cotangents w;
                      <tag>_gx_gap32   max difference of the reference's precision=32 gradient (cotangents cast to float32)
                                       from it;
                    and for the cases with a reconstruct-gradient half:
                      <tag>_gc64_<k>   d<reconstruct(c), y>/dc_k at precision=64, one per coefficient in the build's
                                       flattened order (bands [n, m, m, 2]: the gradient of the (re, im) pair);
                      <tag>_gc_gap32   max difference of the precision=32 gradients from them, over every coefficient.

Both operators are linear, so the gradients do not depend on the point they are taken at: the forward input is zeros.  The
cotangents are not stored; the tests regenerate them from the repo's closed-form generator (scfpyr_grad_cases.py).

The reference is loaded with ref_shim's five shims plus the sixth (callable torch.fft) that make_golden_reconstruct.py
defines; it is imported from there, not repeated.  Fixtures are data only; no reference source is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
import make_golden_reconstruct as mgr  # noqa: E402
import scfpyr_grad_cases as cases  # noqa: E402


def _pyr(ref, height, nbands, precision):
    return ref.SCFpyr_PyTorch(height=height, nbands=nbands, scale_factor=2, device=torch.device("cpu"), precision=precision)


def build_grad(ref, tag, precision):
    size, height, nbands, n = cases.CASES[tag][:4]
    dt = torch.float64 if precision == 64 else torch.float32
    pyr = _pyr(ref, height, nbands, precision)
    x = torch.zeros((n, 1, size, size), dtype=dt, requires_grad=True)
    flat = mgr.flatten(pyr.build(x))
    w = [torch.from_numpy(c).to(dt) for c in cases.coeff_cotangents(tag)]
    assert [tuple(c.shape) for c in flat] == [tuple(t.shape) for t in w]
    (gx,) = torch.autograd.grad(sum((c * t).sum() for c, t in zip(flat, w)), x)
    torch.set_default_dtype(torch.float32)
    return gx.detach().numpy()


def recon_grad(ref, tag, precision):
    size, height, nbands, n = cases.CASES[tag][:4]
    dt = torch.float64 if precision == 64 else torch.float32
    pyr = _pyr(ref, height, nbands, precision)
    flat = [torch.zeros(shp, dtype=dt, requires_grad=True) for shp in cases.shapes(size, height, nbands, n)]
    out = pyr.reconstruct(mgr.nest(flat, height, nbands))
    y = torch.from_numpy(cases.image_cotangent(tag)).to(dt)
    grads = torch.autograd.grad((out * y).sum(), flat)
    torch.set_default_dtype(torch.float32)
    return [g.detach().numpy() for g in grads]


def main():
    ref = ref_shim.load()
    mgr._install_fft_shim()
    out = {}
    for tag, (size, height, nbands, n, key, seed, recon) in cases.CASES.items():
        out["%s_cfg" % tag] = np.array([size, height, nbands, n, 2 + (height - 2) * nbands], dtype=np.int64)
        g64 = build_grad(ref, tag, 64).astype(np.float64)
        g32 = build_grad(ref, tag, 32).astype(np.float64)
        out["%s_gx64" % tag] = g64
        out["%s_gx_gap32" % tag] = np.float64(np.abs(g32 - g64).max())
        msg = "build grad %s, fp32 gap %.2e" % (g64.shape, out["%s_gx_gap32" % tag])
        if recon:
            c64 = recon_grad(ref, tag, 64)
            c32 = recon_grad(ref, tag, 32)
            for k, c in enumerate(c64):
                out["%s_gc64_%d" % (tag, k)] = c.astype(np.float64)
            out["%s_gc_gap32" % tag] = np.float64(max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(c32, c64)))
            msg += ", reconstruct grad %d coefficients, fp32 gap %.2e" % (len(c64), out["%s_gc_gap32" % tag])
        print(tag, size, height, nbands, n, msg)
    np.savez_compressed(os.path.join(HERE, "scfpyr_grad.npz"), **out)


if __name__ == "__main__":
    main()
