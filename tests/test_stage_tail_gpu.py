"""Stage-tail blocks (csrc/nets.hip, MM_STAGE_TAIL): the last bottleneck of conv2_x, conv3_x and conv4_x is read only by the next stage's
1x1 / stride-2 reduce conv and projection shortcut, i.e. at pixels (2i, 2j).  By default its increase conv runs at those pixels alone
(stride 2 over the 3x3 output, the residual read through the engine's strided-residual epilogue) and hands on a compact
[B, ceil(H/2), ceil(W/2), C] tensor that the next block reads at stride 1.  MM_STAGE_TAIL=0 keeps the full-size tails: the parity twin.
Every kept output element is the same sum in the same order: pool5 is equal bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from mimamo_net_amd import weights

pytestmark = pytest.mark.gpu

# the bounds of tests/test_nets_gpu.py::test_resnet50_pool5_vs_oracle
POOL5_RTOL = 1e-5
POOL5_TIGHT_MAX = 2.5e-6
POOL5_TIGHT_MEAN = 2.5e-7

# (H = W of the stage, bottleneck width, output channels) of the three stage tails in the published graph (ceil-mode pool: 56 x 56 at conv2_x)
TAILS = [(56, 64, 256), (28, 128, 512), (14, 256, 1024)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return weights.make_resnet50_state_dict(seed=0)


def _images(n, seed):
    x = weights.det_uniform("rs.img", (n, 3, 224, 224), 0.0, 255.0, seed)
    return x - np.asarray(weights.RESNET50_MEAN, dtype=np.float32)[None, :, None, None]


@pytest.fixture(scope="module")
def xt(dev):
    return torch.from_numpy(_images(3, 1)).to(dev)


@pytest.fixture(scope="module")
def want(oracle, sd):
    """The oracle's pool5 of the three test images (computed once; read-only)."""
    w = oracle.resnet50_pool5(sd, _images(3, 1))
    w.setflags(write=False)
    return w


@pytest.fixture(scope="module")
def make(sd, dev):
    """Extractors by (stage_tail, fuse_inc, fuse_proj, stride_on_first_1x1, ceil_mode, tail_fused); the knobs are read when the handle is created."""
    from mimamo_net_amd.resnet50_extractor import Resnet50_Extractor
    cache = {}

    def get(tail=None, fuse_inc=None, fuse_proj=None, s1=True, ceil=True, tail_fused=None):
        key = (tail, fuse_inc, fuse_proj, s1, ceil, tail_fused)
        if key not in cache:
            mp = pytest.MonkeyPatch()
            try:
                for name, v in (("MM_STAGE_TAIL", tail), ("MM_FUSE_INC", fuse_inc), ("MM_FUSE_PROJ", fuse_proj),
                                ("MM_STAGE_TAIL_FUSED", tail_fused)):
                    if v is None:
                        mp.delenv(name, raising=False)
                    else:
                        mp.setenv(name, str(v))
                cache[key] = Resnet50_Extractor(state_dict=sd, device=dev, stride_on_first_1x1=s1, ceil_mode=ceil)
            finally:
                mp.undo()
        return cache[key]
    yield get
    for net in cache.values():
        net.close()


def _conv_flops(net, x):
    """Executed FLOPs of the conv / GEMM launches of one get_vec (the library's measurement hook, category 0)."""
    from mimamo_net_amd import _lib
    L = _lib.lib()
    ms, work, n = (ctypes.c_double * 5)(), (ctypes.c_double * 5)(), (ctypes.c_int64 * 5)()
    assert L.mm_profile_begin() == 0
    net.get_vec(x)
    assert L.mm_profile_end(ms, work, n) == 0
    return work[0]


@pytest.mark.parametrize("fuse_proj", [0, 1])
@pytest.mark.parametrize("fuse_inc", [0, 3])
def test_stage_tail_twin_equality(make, xt, fuse_inc, fuse_proj):
    """pool5 of the default against MM_STAGE_TAIL=0 for every Winograd mode, at batch 1 (every stage's last workgroup is ragged: 196 / 49 / 16
    tiles against 32-tile workgroups, and M = 784 / 196 / 49 compact rows against 64-row tiles) and batch 3 (workgroups straddle images)."""
    full, tail = make(0, fuse_inc, fuse_proj), make(None, fuse_inc, fuse_proj)
    try:
        for mode in (0, 1, 2, 4, 5):
            full.set_winograd(mode); tail.set_winograd(mode)
            for n in (1, 3):
                x = xt[:n].contiguous()
                a, b = full.get_vec(x), tail.get_vec(x)
                assert torch.isfinite(a).all() and a.std().item() > 0
                assert torch.equal(a, b), (mode, n, (a - b).abs().max().item())
    finally:
        full.set_winograd(True); tail.set_winograd(True)


def test_stage_tail_ragged_spatial_edges(make, xt):
    """ceil_mode=False: conv2_x is 55 x 55 -- clipped right / bottom Winograd tiles, compact 28 x 28 whose last row and column are full-size
    pixel 54 -- conv3_x 28 x 28, conv4_x 14 x 14."""
    full, tail = make(0, ceil=False), make(None, ceil=False)
    try:
        for mode in (1, 0):
            full.set_winograd(mode); tail.set_winograd(mode)
            for n in (1, 3):
                x = xt[:n].contiguous()
                assert torch.equal(full.get_vec(x), tail.get_vec(x)), (mode, n)
    finally:
        full.set_winograd(True); tail.set_winograd(True)
    assert not torch.equal(tail.get_vec(xt), make(None).get_vec(xt))     # floor and ceil mode really differ


def test_stage_tail_leaves_the_stride_on_3x3_graph_alone(make, xt):
    """stride_on_first_1x1=False: the next stage's reduce conv is stride 1 (its 3x3 carries the stride and reads every pixel), so no block is
    a stage tail: equal pool5 and equal executed FLOPs for both knob values."""
    full, tail = make(0, s1=False), make(None, s1=False)
    assert torch.equal(full.get_vec(xt), tail.get_vec(xt))
    assert _conv_flops(full, xt) == _conv_flops(tail, xt)


@pytest.mark.parametrize("fuse_inc", [0, 3])
def test_stage_tail_knob_really_switches_kernels(make, xt, fuse_inc):
    """Executed conv FLOPs (measurement hook), twin minus default = three quarters of the stage-tail increase convs that are launches of their
    own: 2 * mid * cout per dropped pixel, B * (H * H - ceil(H / 2) ** 2) dropped pixels per stage.  With MM_FUSE_INC=0 that is all three
    tails; in the default schedule the conv2_x and conv3_x tails stay inside the fused 3x3 + increase kernel at full size and conv4_x's
    is compacted.  (The 3x3 layers in front of them run all 36 Winograd positions in both forms.)"""
    n = xt.size(0)
    tails = TAILS if fuse_inc == 0 else TAILS[2:]
    want = sum(2.0 * n * (h * h - ((h + 1) // 2) ** 2) * mid * cout for h, mid, cout in tails)
    assert want > 0
    got = _conv_flops(make(0, fuse_inc), xt) - _conv_flops(make(None, fuse_inc), xt)
    assert got == want, (got, want)


def test_stage_tail_default_vs_oracle_and_deterministic(make, xt, want):
    net = make(None)
    first = net.get_vec(xt)
    assert torch.equal(first, net.get_vec(xt))                            # two default runs at batch 3: bit-equal
    got = first.cpu().numpy()
    assert got.shape == (3, 2048)
    scale = np.abs(want).max()
    rel, mean = np.abs(got - want).max() / scale, np.abs(got - want).mean() / scale
    print("stage tail vs oracle: max rel %.3e, mean rel %.3e" % (rel, mean))
    assert rel < POOL5_RTOL * 10, rel
    assert mean < POOL5_RTOL, mean
    assert rel < POOL5_TIGHT_MAX and mean < POOL5_TIGHT_MEAN, ("regression bound", rel, mean)


def test_stage_tail_unfused_tails_opt_in(make, xt, want):
    """MM_STAGE_TAIL_FUSED=0 (opt-in, measured faster): the conv2_x and conv3_x tails leave the fused 3x3 + increase kernel for the plain fused
    3x3 and an increase launch of its own, which is then compacted like conv4_x's.  Bit-equal to its own full-size twin (MM_STAGE_TAIL=0), all
    three increase convs at a quarter of their FLOPs; against the default -- the fused kernel sums the increase contraction in another order --
    and the oracle inside the bounds of test_resnet50_increase_conv_inside_the_fused_winograd_kernel."""
    full, tail, default = make(0, tail_fused=0), make(None, tail_fused=0), make(None)
    for n in (1, 3):
        x = xt[:n].contiguous()
        assert torch.equal(full.get_vec(x), tail.get_vec(x)), n
    n = xt.size(0)
    want_fl = sum(2.0 * n * (h * h - ((h + 1) // 2) ** 2) * mid * cout for h, mid, cout in TAILS)
    assert _conv_flops(full, xt) - _conv_flops(tail, xt) == want_fl
    scale = np.abs(want).max()
    a, b = tail.get_vec(xt).cpu().numpy(), default.get_vec(xt).cpu().numpy()
    assert not np.array_equal(a, b)                                       # the knob really switches the schedule
    d = np.abs(a - b).max() / scale
    rel, mean = np.abs(a - want).max() / scale, np.abs(a - want).mean() / scale
    print("unfused tails vs default max rel %.3e; vs oracle max rel %.3e, mean rel %.3e" % (d, rel, mean))
    assert d < 1e-5, d
    assert rel < POOL5_RTOL * 10 and mean < POOL5_RTOL
    assert rel < POOL5_TIGHT_MAX and mean < POOL5_TIGHT_MEAN, ("regression bound", rel, mean)
