"""Cotangents of the SCFpyr_PyTorch gradient fixture (tests/golden/scfpyr_grad.npz), regenerated from the repo's closed-form
generator exactly as tests/golden/make_golden_scfpyr_grad.py generated them; the fixture stores only the reference's gradients.
Shared by test_scfpyr_autograd_cpu.py and test_scfpyr_autograd_gpu.py.

Both operators are linear, so a gradient depends only on the geometry and the cotangent, not on the forward input.  Every
case has a build-gradient half (cotangents on every coefficient -> the image gradient); the cases marked `recon` also have a
reconstruct-gradient half (a cotangent on the image -> one gradient per coefficient).  The geometries are those of the
reconstruct fixture (scfpyr_recon_cases.py; its case h repeats e's geometry and is left out); the largest grids carry no
reconstruct-gradient half, whose per-coefficient gradients would dominate the file."""
import numpy as np

from mimamo_net_amd import weights

CASES = {
    # tag: (size, height, nbands, n_images, det_uniform key, seed, recon)
    "a": (96, 4, 2, 1, "scf.grad.a", 21, False),
    "b": (32, 3, 4, 2, "scf.grad.b", 22, True),
    "c": (32, 3, 3, 1, "scf.grad.c", 23, True),
    "d": (50, 3, 2, 1, "scf.grad.d", 24, True),
    "e": (75, 4, 2, 1, "scf.grad.e", 25, True),
    "f": (84, 4, 2, 1, "scf.grad.f", 26, False),
    "g": (130, 5, 2, 1, "scf.grad.g", 27, False),     # side above 96: the transforms' scratch path
    "i": (50, 3, 3, 2, "scf.grad.i", 28, False),
    "j": (32, 2, 2, 2, "scf.grad.j", 29, True),       # height 2: [hi, lo]; the reference needs N == nbands here
}
RECON_CASES = [t for t, c in CASES.items() if c[6]]


def shapes(size, height, nbands, n):
    out = [(n, size, size)]
    s = size
    for _ in range(height - 2):
        out += [(n, s, s, 2)] * nbands
        s = int(np.ceil((s - 0.5) / 2))
    return out + [(n, s, s)]


def coeff_cotangents(tag):
    """The build-gradient half's upstream gradients, one per coefficient in the build's flattened order (float64)."""
    size, height, nbands, n, key, seed, _ = CASES[tag]
    return [weights.det_uniform("%s.c%d" % (key, k), shp, -1.0, 1.0, seed).astype(np.float64)
            for k, shp in enumerate(shapes(size, height, nbands, n))]


def image_cotangent(tag):
    """The reconstruct-gradient half's upstream gradient, [n, size, size] (float64)."""
    size, height, nbands, n, key, seed, _ = CASES[tag]
    return weights.det_uniform("%s.y" % key, (n, size, size), -1.0, 1.0, seed).astype(np.float64)


def check_cfg(g, tag):
    size, height, nbands, n = CASES[tag][:4]
    assert [int(v) for v in g[tag + "_cfg"]] == [size, height, nbands, n, 2 + (height - 2) * nbands]
