"""Inputs of the SCFpyr_PyTorch.reconstruct fixture cases (tests/golden/scfpyr_reconstruct.npz), regenerated from the repo's
closed-form generator exactly as tests/golden/make_golden_reconstruct.py generated them; the fixture stores only the reference's
outputs.  Shared by test_scfpyr_reconstruct_cpu.py and test_scfpyr_reconstruct_gpu.py."""
import numpy as np

from mimamo_net_amd import weights

CASES = {
    # tag: (size, height, nbands, n_images, det_uniform key, seed, kind)  -- make_golden_reconstruct.CASES
    "a": (96, 4, 2, 1, "scf.a", 8, "image"),
    "b": (32, 3, 4, 2, "scf.b", 9, "image"),
    "c": (32, 3, 3, 1, "scf.c", 10, "image"),
    "d": (50, 3, 2, 1, "scf.d", 11, "image"),
    "e": (75, 4, 2, 1, "scf.e", 12, "image"),
    "f": (84, 4, 2, 1, "scf.f", 13, "image"),
    "g": (130, 5, 2, 1, "scf.g", 14, "image"),
    "h": (75, 4, 2, 1, "scf.e", 12, "edited"),
    "i": (50, 3, 3, 2, "scf.recon.i", 15, "random"),
    "j": (32, 2, 2, 2, "scf.j", 16, "image"),
}
IMAGE_CASES = [t for t, c in CASES.items() if c[6] == "image"]


def shapes(size, height, nbands, n):
    out = [(n, size, size)]
    s = size
    for _ in range(height - 2):
        out += [(n, s, s, 2)] * nbands
        s = int(np.ceil((s - 0.5) / 2))
    return out + [(n, s, s)]


def image(tag):
    size, height, nbands, n, key, seed, kind = CASES[tag]
    assert kind != "random"
    return weights.det_uniform(key, (n, 1, size, size), 0.0, 1.0, seed).astype(np.float64)


def inputs(tag, g, build):
    """The case's float64 coefficients, flattened in the build's output order.  `build(x [n,1,s,s] float64)` must return the
    pyramid of x flattened the same way (the library's build: pinned to the reference's by G8)."""
    size, height, nbands, n, key, seed, kind = CASES[tag]
    assert [int(v) for v in g[tag + "_cfg"]] == [size, height, nbands, n, 2 + (height - 2) * nbands]
    if kind == "random":
        return [weights.det_uniform("%s.%d" % (key, k), shp, -1.0, 1.0, seed).astype(np.float64)
                for k, shp in enumerate(shapes(size, height, nbands, n))]
    flat = [np.asarray(c, dtype=np.float64) for c in build(image(tag))]
    if kind == "edited":   # bands times e^{i theta_k}, hi-pass residual halved, low-pass residual + 0.1
        for k, t in enumerate(g[tag + "_theta"]):
            z = (flat[1 + k][..., 0] + 1j * flat[1 + k][..., 1]) * np.exp(1j * t)
            flat[1 + k] = np.stack([z.real, z.imag], -1)
        flat[0] = flat[0] * 0.5
        flat[-1] = flat[-1] + 0.1
    assert [c.shape for c in flat] == shapes(size, height, nbands, n)
    return flat
