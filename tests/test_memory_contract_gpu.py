"""GPU: the memory contract of every workspace-taking entry point, through the C ABI so that the test owns every buffer.

Each case runs the call once per entry of guarded.FILLS with
  - a workspace of exactly mm_*_workspace_bytes() bytes, pre-filled (zeros / NaN / +3e38 / -3e38), between guards;
  - every input between NaN guards (a load past a ragged tile or a padded channel group meets a NaN, not a lucky zero);
  - every output between guards and pre-filled with the output sentinel;
and asserts: MM_OK; all guards intact; outputs fully written inside their declared window and untouched outside it; outputs
finite and bit-identical across the four fills; the NaN-fill output within the existing tolerance of the high-precision
reference of that entry point (so this is not a self-consistency check); MM_ERR_WORKSPACE at workspace_bytes - 1 with
nothing written.  The last section overwrites the workspaces the Python classes cache per stream.
"""
import ctypes

import numpy as np
import pytest
import torch

import scfpyr_grad_cases as scf_cases
from guarded import FILLS, SENTINEL, assert_fully_written, assert_untouched, guarded
from mimamo_net_amd import _lib, synthetic, weights
from test_nets_gpu import OUT_ATOL, POOL5_RTOL, POOL5_TIGHT_MAX, POOL5_TIGHT_MEAN, _images
from test_phase_gpu import PHASE_ATOL, PHASE_P9999, _phase_err, _tight

pytestmark = pytest.mark.gpu

F32, F64, I32 = torch.float32, torch.float64, torch.int32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _workspace(nbytes, dev, fill, dtype=F32):
    """Exactly nbytes of workspace between guards, every element = fill."""
    item = 4 if dtype == F32 else 8
    assert nbytes > 0 and nbytes % item == 0, nbytes
    return guarded((nbytes // item,), dtype, dev, fill)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64)


def _same_across_fills(outs, what="output"):
    """outs: {fill name: tensor or list of tensors}; every entry finite and torch.equal to the zero-fill one."""
    as_list = lambda v: list(v) if isinstance(v, (list, tuple)) else [v]
    base = as_list(outs["zeros"])
    for name, got in outs.items():
        for k, (a, b) in enumerate(zip(as_list(got), base)):
            assert torch.isfinite(a).all(), "%s %d is not finite with a %s-filled workspace" % (what, k, name)
            assert torch.equal(a, b), "%s %d depends on what the workspace held: fill %s differs from zeros in %d elements (max %.3e)" % (
                what, k, name, int((a != b).sum()), float((a - b).abs().max()))


def _refused(call, need, dev, outputs, dtype=F32, inout=()):
    """The call with workspace_bytes - 1: MM_ERR_WORKSPACE, no output element written, no workspace element written, the in/out
    buffers unchanged.  call(ws_ptr, ws_bytes) -> status; outputs: [(tensor, check)] pre-filled with the output sentinel."""
    ws, ck = _workspace(need, dev, FILLS["nan"], dtype)
    before = _bits(ws).clone()
    kept = [_bits(t).clone() for t in inout]
    assert call(_lib.ptr(ws), need - 1) == _lib.MM_ERR_WORKSPACE
    torch.cuda.synchronize()
    ck("workspace")
    assert torch.equal(_bits(ws), before), "a refused call wrote its workspace"
    for t, c in outputs:
        c("output")
        assert_untouched(t)
    for t, k in zip(inout, kept):
        assert torch.equal(_bits(t), k), "a refused call wrote an in/out buffer"


# ======================================================================================================================
# ResNet50 trunk
# ======================================================================================================================
GRAPHS = {"published": (1, 1), "floor": (0, 0)}     # (stride_on_first_1x1, ceil_mode); floor: 55 x 55 maps, 9075 pooled pixels at N = 3


@pytest.fixture(scope="module")
def trunks(pkg, dev, oracle):
    """One native handle per graph, five images and the oracle's pool5 of all five per graph (computed on first use, shared)."""
    L = _lib.lib()
    sd = weights.make_resnet50_state_dict(seed=0)
    blob = weights.resnet50_blob(sd)
    x = _images(5, 31)
    handles, want = {}, {}
    for name, (s1, cm) in GRAPHS.items():
        h = ctypes.c_void_p()
        assert L.mm_resnet50_create(ctypes.byref(h), blob.ctypes.data_as(ctypes.c_void_p), blob.size, s1, cm, 1e-5) == 0
        handles[name] = h

    def reference(name):
        if name not in want:
            s1, cm = GRAPHS[name]
            want[name] = oracle.resnet50_pool5(sd, x, stride_on_first_1x1=bool(s1), ceil_mode=bool(cm))
        return want[name]
    yield handles, x, reference
    for h in handles.values():
        L.mm_resnet50_destroy(h)


RESNET_CASES = {
    # name: (batch, input layout, winograd mode, precision mode, batch the workspace is sized and declared for)
    "n1": (1, 1, 1, 0, None),
    "n3": (3, 1, 1, 0, None),            # winograd mode 1 (the default schedule) at batch 3
    "n5": (5, 1, 1, 0, None),
    "n3-direct": (3, 1, 0, 0, None),
    "n3-wino2": (3, 1, 2, 0, None),
    "n3-wino4": (3, 1, 4, 0, None),
    "n3-nhwc4": (3, 0, 1, 0, None),
    "n3-bordered3": (3, 2, 1, 0, None),
    "n3-bf16x3": (3, 1, 1, 1, None),
    "n3-in-n5-workspace": (3, 1, 1, 0, 5),
}


def _trunk_input(x, layout):
    if layout == 1:
        return np.ascontiguousarray(x)
    nhwc = x.transpose(0, 2, 3, 1)
    if layout == 0:
        out = np.zeros((x.shape[0], 224, 224, 4), dtype=np.float32)
        out[..., :3] = nhwc
        return out
    out = np.zeros((x.shape[0], 230, 230, 3), dtype=np.float32)      # layout 2: the caller supplies the stem's zero border
    out[:, 3:227, 3:227, :] = nhwc
    return out


@pytest.mark.parametrize("case", sorted(RESNET_CASES))
@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_resnet50_forward_memory_contract(trunks, dev, graph, case):
    L = _lib.lib()
    handles, x, reference = trunks
    h = handles[graph]
    n, layout, wino, prec, ws_n = RESNET_CASES[case]
    xin = _trunk_input(x[:n], layout)
    need = L.mm_resnet50_workspace_bytes(h, n)
    declared = L.mm_resnet50_workspace_bytes(h, ws_n or n)
    assert 0 < need <= declared
    assert L.mm_resnet50_set_winograd(h, wino) == 0 and L.mm_resnet50_set_precision(h, prec) == 0
    try:
        img, ck_img = guarded(xin.shape, F32, dev, xin)
        outs = {}
        for fname, fill in FILLS.items():
            out, ck_out = guarded((n, 2048), F32, dev, SENTINEL)
            ws, ck_ws = _workspace(declared, dev, fill)
            rc = L.mm_resnet50_forward(h, _lib.ptr(img), layout, n, _lib.ptr(out), _lib.ptr(ws), declared, _lib.current_stream())
            torch.cuda.synchronize()
            assert rc == _lib.MM_OK, (fname, rc)
            ck_ws("workspace (%s)" % fname), ck_img("images"), ck_out("pool5")
            assert_fully_written(out)
            outs[fname] = out.clone()
            del ws, ck_ws
        assert torch.equal(img, torch.from_numpy(xin).to(dev))           # the input is read-only
        _same_across_fills(outs, "pool5")
        want = reference(graph)[:n]
        got = outs["nan"].cpu().numpy()
        scale = np.abs(want).max()
        mx, mean = np.abs(got - want).max() / scale, np.abs(got - want).mean() / scale
        print("%s %s: pool5 max rel %.2e mean rel %.2e" % (graph, case, mx, mean))
        assert mx < POOL5_RTOL * 10 and mean < POOL5_RTOL, (mx, mean)
        if prec == 0 and layout != 0:       # the tight regression bounds belong to the fp32 path on the K = 168 stem, as in test_nets_gpu.py
            assert mx < POOL5_TIGHT_MAX and mean < POOL5_TIGHT_MEAN, ("regression bound", mx, mean)
        out, ck_out = guarded((n, 2048), F32, dev, SENTINEL)
        _refused(lambda w, b: L.mm_resnet50_forward(h, _lib.ptr(img), layout, n, _lib.ptr(out), w, b, _lib.current_stream()),
                 need, dev, [(out, ck_out)])
    finally:
        L.mm_resnet50_set_winograd(h, 1)
        L.mm_resnet50_set_precision(h, 0)


# ======================================================================================================================
# Two-stream head
# ======================================================================================================================
HEADS = {
    # name: (state_dict seed, mlp units, num_phase, regression bound next to OUT_ATOL -- those of the existing tests of that configuration)
    "published": (3, (2048, 256, 256), 12, 2e-5),
    "num_phase5": (11, (2048, 256, 256), 5, 3e-5),       # 10 channels padded to 12: zero channels meet zero weights
    "num_phase40": (11, (2048, 256, 256), 40, 3e-5),     # 64 + 80 > 128 channels: the concat layer runs in the direct form
    "mlp512": (9, (2048, 512, 256), 12, 2e-5),
}
HEAD_CASES = [("published", bs, T, layout) for (bs, T) in ((1, 1), (3, 5), (2, 33)) for layout in (0, 1, 2)] + \
             [("num_phase5", 3, 5, 0), ("num_phase40", 3, 5, 0), ("mlp512", 3, 5, 0)]


@pytest.fixture(scope="module")
def heads(pkg, dev, oracle):
    L = _lib.lib()
    made, refs = {}, {}

    def get(name):
        if name not in made:
            seed, units, nph, _ = HEADS[name]
            sd = weights.make_two_stream_state_dict(seed=seed, num_phase=nph, mlp_units=list(units))
            blob = weights.two_stream_blob(sd, units)
            h = ctypes.c_void_p()
            cu = (ctypes.c_int * len(units))(*units)
            assert L.mm_head_create_cfg(ctypes.byref(h), blob.ctypes.data_as(ctypes.c_void_p), blob.size, len(units), cu, nph) == 0
            made[name] = (h, sd)
        return made[name]

    def inputs_and_reference(name, bs, T):
        """Shared by the three layouts of a (head, bs, T): inputs and the float64 oracle's output."""
        key = (name, bs, T)
        if key not in refs:
            _, units, nph, _ = HEADS[name]
            p0 = weights.det_uniform("mc.p0", (bs, T, 2 * nph, 48, 48), -1.5, 1.5, 40 + bs)
            p1 = weights.det_uniform("mc.p1", (bs, T, 2 * nph, 24, 24), -1.5, 1.5, 40 + bs)
            rgb = weights.det_uniform("mc.rgb", (bs, T, units[0]), 0.0, 2.0, 40 + bs)
            refs[key] = (p0, p1, rgb, oracle.two_stream_forward(get(name)[1], p0, p1, rgb, dtype=np.float64))
        return refs[key]
    yield get, inputs_and_reference
    for h, _ in made.values():
        L.mm_head_destroy(h)


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "%s-bs%d-T%d-layout%d" % c)
def test_head_forward_memory_contract(heads, dev, case):
    L = _lib.lib()
    name, bs, T, layout = case
    get, inputs_and_reference = heads
    h = get(name)[0]
    p0, p1, rgb, want = inputs_and_reference(name, bs, T)
    N, C = bs * T, p0.shape[2]
    if layout:
        p0 = np.ascontiguousarray(p0.reshape(N, C, 48, 48).transpose(0, 2, 3, 1))
        p1 = np.ascontiguousarray(p1.reshape(N, C, 24, 24).transpose(0, 2, 3, 1))
    t0, ck0 = guarded(p0.shape, F32, dev, p0)
    trgb, ckr = guarded(rgb.shape, F32, dev, rgb)
    level1 = torch.from_numpy(p1).to(dev)
    need = L.mm_head_workspace_bytes(h, bs, T)
    outs, cats = {}, {}
    for fname, fill in FILLS.items():
        if layout == 2:
            # the caller's concat buffer [N,24,24,64+C]: level-1 phase at channels 64.., the call completes channels 0..63 in place
            t1, ck1 = guarded((N, 24, 24, 64 + C), F32, dev, fill)
            t1[..., 64:] = level1
        else:
            t1, ck1 = guarded(p1.shape, F32, dev, p1)
        out, ck_out = guarded((bs, T, 2), F32, dev, SENTINEL)
        ws, ck_ws = _workspace(need, dev, fill)
        rc = L.mm_head_forward(h, _lib.ptr(t0), _lib.ptr(t1), layout, _lib.ptr(trgb), bs, T, _lib.ptr(out), _lib.ptr(ws), need,
                               _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == _lib.MM_OK, (fname, rc)
        ck_ws("workspace (%s)" % fname), ck0("phase_0"), ck1("phase_1"), ckr("rgb"), ck_out("out")
        assert_fully_written(out)
        if layout == 2:
            assert torch.equal(_bits(t1[..., 64:]), _bits(level1)), "channels 64.. of the caller's concat buffer changed"
            cats[fname] = t1[..., :64].clone()
        else:
            assert torch.equal(_bits(t1), _bits(level1.view(t1.shape)))
        outs[fname] = out.clone()
        del ws, ck_ws
    assert torch.equal(t0, torch.from_numpy(p0).to(dev)) and torch.equal(trgb, torch.from_numpy(rgb).to(dev))
    _same_across_fills(outs, "valence/arousal")
    if layout == 2:
        _same_across_fills(cats, "channels 0..63 of the concat buffer")       # overwritten whatever they held
    err = np.abs(outs["nan"].cpu().numpy() - want).max()
    print("%s bs %d T %d layout %d: max |out - float64 oracle| %.2e" % (name, bs, T, layout, err))
    assert err < OUT_ATOL and err < HEADS[name][3], err
    out, ck_out = guarded((bs, T, 2), F32, dev, SENTINEL)
    _refused(lambda w, b: L.mm_head_forward(h, _lib.ptr(t0), _lib.ptr(t1), layout, _lib.ptr(trgb), bs, T, _lib.ptr(out), w, b,
                                            _lib.current_stream()),
             need, dev, [(out, ck_out)], inout=[t1])


# ======================================================================================================================
# Fused phase stage
# ======================================================================================================================
PHASE_LAYOUTS = {
    # name: ((nhwc, cstride, coffset) of out0, the same of out1)
    "nchw": ((0, 0, 0), (0, 0, 0)),
    "nhwc24": ((1, 24, 0), (1, 24, 0)),
    "nhwc32+88": ((1, 32, 4), (1, 88, 64)),       # out1 as the head's concat buffer takes it: 96 of 352 bytes per pixel
    "nhwc+nchw": ((1, 24, 0), (0, 0, 0)),         # mixed layouts: one launch per level
}
# frame counts at which the dispatch of pyramid_frames.hip / pyramid_wave.hip changes
PHASE_N = [1, 13, 40,       # the three-wave kernel
           513,             # wave kernel, four waves per workgroup; the last workgroup holds one frame
           1027,            # eight waves per workgroup, ragged
           2048 + 3,        # a whole round on the wave kernel + three frames on the three-wave kernel
           2048 + 515]      # a round + a wave-kernel remainder


@pytest.fixture(scope="module")
def phase(pkg, dev, oracle):
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.mm_pyramid_create(ctypes.byref(h), 48, 4, 2, 2) == 0
    small = synthetic.textured_gray(40, 48, seed=55)          # test_dedup_fast_path_matches_drop_in's clip: the oracle stays inside the flip cap on it
    base = torch.from_numpy(synthetic.textured_gray(64, 48, seed=300)).to(dev)
    refs = {}

    def oracle_ref(n):
        if n not in refs:
            ids = oracle.window_ids(0, n, n).astype(np.int32)
            refs[n] = (ids, oracle.phase_diff_from_frames(small[:n], ids))
        return refs[n]
    yield h, small, base, oracle_ref, {}
    L.mm_pyramid_destroy(h)


def _clip_windows(lo, hi, dev):
    """Window ids of the clip of frames [lo, hi): frame t's window is t-6..t+6 clamped into the clip (as the load test builds them)."""
    t = torch.arange(lo, hi, device=dev)[:, None] + torch.arange(-6, 7, device=dev)[None, :]
    return torch.clamp(t, lo, hi - 1).int().contiguous()


def _phase_out(J, W, spec, dev):
    nhwc, cs, _ = spec
    return guarded((J, W, W, cs) if nhwc else (J, 24, W, W), F32, dev, SENTINEL)


def _phase_nchw(t, spec):
    nhwc, _, co = spec
    return t[..., co:co + 24].permute(0, 3, 1, 2).contiguous() if nhwc else t.clone()


def _check_phase_out(t, ck, spec, what):
    ck(what)
    if spec[0]:
        assert_fully_written(t, (spec[2], spec[2] + 24))
        assert_untouched(t, (spec[2], spec[2] + 24))           # the other channels of every row
    else:
        assert_fully_written(t)


def _phase_call(h, frames, ids, layout, fill, dev, keep_ws=False):
    """One guarded mm_phase_diff_frames -> (out0, out1) as NCHW copies (and the workspace when keep_ws)."""
    L = _lib.lib()
    s0, s1 = PHASE_LAYOUTS[layout]
    n, J = frames.shape[0], ids.shape[0]
    f, ckf = guarded(frames.shape, F32, dev, frames)
    i, cki = guarded(ids.shape, I32, dev, ids)
    o0, ck0 = _phase_out(J, 48, s0, dev)
    o1, ck1 = _phase_out(J, 24, s1, dev)
    need = L.mm_phase_workspace_bytes(h, n)
    ws, ckw = _workspace(need, dev, fill)
    rc = L.mm_phase_diff_frames(h, _lib.ptr(f), n, _lib.ptr(i), J, _lib.ptr(o0), *s0, _lib.ptr(o1), *s1, _lib.ptr(ws), need,
                                _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == _lib.MM_OK, rc
    ckw("workspace"), ckf("frames"), cki("ids")
    _check_phase_out(o0, ck0, s0, "out0")
    _check_phase_out(o1, ck1, s1, "out1")
    assert torch.equal(f, frames) and torch.equal(i, ids)
    res = (_phase_nchw(o0, s0), _phase_nchw(o1, s1))
    return res + (ws,) if keep_ws else res


@pytest.mark.parametrize("layout", sorted(PHASE_LAYOUTS))
@pytest.mark.parametrize("n", PHASE_N)
def test_phase_diff_frames_memory_contract(phase, dev, n, layout):
    L = _lib.lib()
    h, small, base, oracle_ref, alone = phase
    if n <= 40:
        ids_np, want = oracle_ref(n)
        frames, ids = torch.from_numpy(small[:n].copy()).to(dev), torch.from_numpy(ids_np).to(dev)
        clips = []
    else:
        # 64 frames repeated on the device; windows of the first clip, of the clip that starts at frame 2048 (the first frames past a
        # whole round of the wave kernel) and of the last, partial clip -- every clip is a prefix of the first
        frames = base.repeat((n + 63) // 64, 1, 1)[:n].contiguous()
        clips = sorted(set([(0, 64), (64 * ((n - 1) // 64), n)] + ([(2048, min(2112, n))] if n > 2048 else [])))
        ids = torch.cat([_clip_windows(lo, hi, dev) for lo, hi in clips])
    outs = {fname: _phase_call(h, frames, ids, layout, fill, dev) for fname, fill in FILLS.items()}
    _same_across_fills(outs, "phase difference")
    got0, got1 = outs["nan"]
    if n <= 40:
        for got, w in ((got0, want[0]), (got1, want[1])):
            mx, p9999, flips = _phase_err(got.cpu().numpy(), w)
            assert mx < PHASE_ATOL and p9999 < PHASE_P9999 and flips <= 4, (mx, p9999, flips)
            _tight(mx, p9999, flips)
    else:
        row = 0
        for lo, hi in clips:       # rows bit-equal to the same clip computed alone (a prefix of the 64 base frames)
            k = hi - lo
            if (k, layout) not in alone:
                alone[(k, layout)] = _phase_call(h, base[:k].contiguous(), _clip_windows(0, k, dev), layout, 0.0, dev)
            a0, a1 = alone[(k, layout)]
            assert torch.equal(got0[row:row + k], a0) and torch.equal(got1[row:row + k], a1), (n, lo, hi)
            row += k
    s0, s1 = PHASE_LAYOUTS[layout]
    J = ids.shape[0]
    o0, ck0 = _phase_out(J, 48, s0, dev)
    o1, ck1 = _phase_out(J, 24, s1, dev)
    _refused(lambda w, b: L.mm_phase_diff_frames(h, _lib.ptr(frames), n, _lib.ptr(ids), J, _lib.ptr(o0), *s0, _lib.ptr(o1), *s1, w, b,
                                                 _lib.current_stream()),
             L.mm_phase_workspace_bytes(h, n), dev, [(o0, ck0), (o1, ck1)])


def test_phase_diff_planes_on_the_planes_left_in_the_workspace(phase, dev):
    """mm_phase_diff_planes on guarded copies of the per-frame planes mm_phase_diff_frames left in its workspace: the same bits."""
    L = _lib.lib()
    h, small, _, oracle_ref, _ = phase
    n = 13
    ids = torch.from_numpy(oracle_ref(n)[0]).to(dev)
    frames = torch.from_numpy(small[:n].copy()).to(dev)
    want0, want1, ws = _phase_call(h, frames, ids, "nchw", FILLS["nan"], dev, keep_ws=True)
    n1 = n * 2 * 4 * 48 * 48
    i, cki = guarded(ids.shape, I32, dev, ids)
    for W, src, want in ((48, ws[:n1], want0), (24, ws[n1:], want1)):
        assert src.numel() == n * 2 * 4 * W * W
        planes, ckp = guarded((n, 2, 4, W, W), F32, dev, src.view(n, 2, 4, W, W))
        out, cko = guarded((n, 24, W, W), F32, dev, SENTINEL)
        rc = L.mm_phase_diff_planes(h, _lib.ptr(planes), n, _lib.ptr(i), n, W, _lib.ptr(out), 0, 0, 0, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == _lib.MM_OK
        ckp("planes"), cki("ids"), cko("out")
        assert_fully_written(out)
        assert torch.isfinite(out).all() and torch.equal(out, want)
        out, cko = guarded((n, W, W, 88), F32, dev, SENTINEL)                   # and into a channel window
        rc = L.mm_phase_diff_planes(h, _lib.ptr(planes), n, _lib.ptr(i), n, W, _lib.ptr(out), 1, 88, 64, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == _lib.MM_OK
        _check_phase_out(out, cko, (1, 88, 64), "out")
        ckp("planes")
        assert torch.equal(out[..., 64:].permute(0, 3, 1, 2), want)


# ======================================================================================================================
# Generic extract (with the denoised phase)
# ======================================================================================================================
GENERIC_PLANES = [(64, 64),      # 4096 pixels: the limit of the LDS kernel
                  (64, 65),      # the first size that needs the workspace
                  (7, 5),        # narrower than the 11-tap blur
                  (30, 50)]      # non-square
GENERIC_SETS = 3
# det_uniform seed per (R, C, P), see the docstring of the test
GENERIC_SEEDS = {(64, 64, 2): 1, (64, 64, 13): 1, (64, 65, 2): 1, (64, 65, 13): 1, (7, 5, 2): 1, (7, 5, 13): 1, (30, 50, 2): 1,
                 (30, 50, 13): 1}


def _generic_coeff(R, C, P):
    """Coefficients of the magnitude of real band coefficients (|c| ~ 1e-2 .. 1e-1, test_phase_gpu.py's COEFF_ATOL note)."""
    return weights.det_uniform("mc.coeff", (GENERIC_SETS, P, R, C, 2), -1.0, 1.0, GENERIC_SEEDS[(R, C, P)]) * np.float32(0.05)


@pytest.mark.parametrize("P", [2, 13])
@pytest.mark.parametrize("plane", GENERIC_PLANES, ids=lambda p: "%dx%d" % p)
def test_phase_extract_generic_memory_contract(pkg, oracle, dev, plane, P):
    """Seeds.  Random coefficients have phase steps all over (-2 pi, 2 pi), so a step within rounding of +-pi would make fp32 and
    float64 unwrap differently (a 2 pi branch flip that the blur then smears over 11 x 11 pixels and every later frame).  The fp32 and
    float64 oracles were run against each other on the CPU host for each (plane, P), seeds tried from 1 upwards: seed 1 was kept
    for all eight cases, with 0 flips of the oracle against itself in both outputs everywhere and max |fp32 - float64|
        64x64: P 2 1.3e-6, P 13 1.3e-5     64x65: P 2 1.4e-6, P 13 1.4e-5     7x5: P 2 5.0e-7, P 13 6.7e-6     30x50: P 2 9.7e-7, P 13 1.1e-5
    (differences / denoised phase, the larger of the two), well inside the existing generic tests' cap of 2 flips and PHASE_ATOL."""
    L = _lib.lib()
    R, C = plane
    S = GENERIC_SETS
    c = _generic_coeff(R, C, P)
    coeff, ckc = guarded(c.shape, F32, dev, c)
    need = L.mm_phase_extract_generic_workspace_bytes(S, P, R, C)
    fits_lds = need == 0
    assert fits_lds == (R * C <= 4096)
    if fits_lds:
        need = S * R * C * 8 * 4          # a sufficient workspace selects the workspace kernel whatever the plane size
    call = lambda o, d, w, b: L.mm_phase_extract_generic_ws(_lib.ptr(coeff), S, P, R, C, _lib.ptr(o), _lib.ptr(d), w, b, _lib.current_stream())
    outs = {}
    for fname, fill in FILLS.items():
        out, cko = guarded((S, P - 1, R, C), F32, dev, SENTINEL)
        den, ckd = guarded((S, P, R, C), F32, dev, SENTINEL)
        ws, ckw = _workspace(need, dev, fill)
        rc = call(out, den, _lib.ptr(ws), need)
        torch.cuda.synchronize()
        assert rc == _lib.MM_OK, (fname, rc)
        ckw("workspace (%s)" % fname), ckc("coeff"), cko("out"), ckd("denoised")
        assert_fully_written(out), assert_fully_written(den)
        outs[fname] = [out.clone(), den.clone()]
    assert torch.equal(coeff, torch.from_numpy(c).to(dev))
    _same_across_fills(outs, "generic extract")
    if fits_lds:     # no workspace: the LDS kernel, the same bits
        out, cko = guarded((S, P - 1, R, C), F32, dev, SENTINEL)
        den, ckd = guarded((S, P, R, C), F32, dev, SENTINEL)
        assert call(out, den, None, 0) == _lib.MM_OK
        torch.cuda.synchronize()
        ckc("coeff"), cko("out"), ckd("denoised")
        assert_fully_written(out), assert_fully_written(den)
        assert torch.equal(out, outs["nan"][0]) and torch.equal(den, outs["nan"][1])
    want_d = oracle.extract(c[None], dtype=np.float64)[0]
    want_p = oracle.extract_phase(c[None], return_phase=True, dtype=np.float64)[0]
    for got, want in ((outs["nan"][0], want_d), (outs["nan"][1], want_p)):
        mx, p9999, flips = _phase_err(got.cpu().numpy(), want)
        assert got.shape == want.shape and mx < PHASE_ATOL and p9999 < PHASE_P9999 and flips <= 2, (mx, p9999, flips)
    out, cko = guarded((S, P - 1, R, C), F32, dev, SENTINEL)
    den, ckd = guarded((S, P, R, C), F32, dev, SENTINEL)
    _refused(lambda w, b: call(out, den, w, b), need, dev, [(out, cko), (den, ckd)])


# ======================================================================================================================
# General pyramid: build, reconstruct and the two adjoints
# ======================================================================================================================
SCF_CONFIGS = [(32, 3, 4), (96, 4, 2),      # 96: the last side whose transforms stay in LDS
               (97, 4, 2)]                  # the first that uses the scratch plane of the workspace; odd


@pytest.fixture(scope="module")
def scf(pkg, dev):
    L = _lib.lib()
    made = {}

    def get(size, height, nbands, n):
        key = (size, height, nbands)
        if key not in made:
            h = ctypes.c_void_p()
            assert L.mm_scfpyr_create(ctypes.byref(h), size, height, nbands, 2) == 0
            made[key] = h
        h = made[key]
        side, cplx = ctypes.c_int(), ctypes.c_int()
        shapes = []
        for k in range(L.mm_scfpyr_num_outputs(h)):
            assert L.mm_scfpyr_output_info(h, k, ctypes.byref(side), ctypes.byref(cplx)) == 0
            shapes.append((n, side.value, side.value, 2) if cplx.value else (n, side.value, side.value))
        assert shapes == scf_cases.shapes(size, height, nbands, n)
        return h, shapes
    yield get
    for h in made.values():
        L.mm_scfpyr_destroy(h)


def _host_table(fn, size, height, nbands, index):
    side, cp = ctypes.c_int(), ctypes.c_int()
    assert fn(size, height, nbands, 2, index, None, ctypes.byref(side), ctypes.byref(cp)) == 0
    t = np.zeros((side.value, side.value, 2))
    assert fn(size, height, nbands, 2, index, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(side), ctypes.byref(cp)) == 0
    return t[..., 0] + 1j * t[..., 1]


def _host_reconstruct(flat, size, height, nbands):
    """The reference's reconstruction from the library's host-side float64 multipliers and numpy's FFT, in the convention of
    include/mimamo_hip.h -- test_scfpyr_reconstruct_cpu.py pins exactly this evaluation to the real reference's float64 outputs
    (tests/golden/scfpyr_reconstruct.npz) within 1e-12 on every fixture geometry."""
    L = _lib.lib()
    n = flat[0].shape[0]
    S = np.zeros((n, size, size), dtype=np.complex128)
    for k, c in enumerate(flat):
        Rk = _host_table(L.mm_scfpyr_host_recon_table, size, height, nbands, k)
        c = c.astype(np.float64)
        if c.ndim == 4:
            c = c[..., 0] + 1j * c[..., 1]
        m = Rk.shape[0]
        idx = np.arange(m)
        fa = np.where(idx < (m + 1) // 2, idx, idx - m) % size
        S[:, fa[:, None], fa[None, :]] += np.fft.fft2(c) * Rk
    return (np.fft.ifft2(S) * (size * size)).real


def _scf_rand(name, shape, seed, dt):
    """Values in [-1, 1) that are exact in fp32 (24 random bits), so both precisions see the same numbers."""
    return weights.det_uniform(name, shape, -1.0, 1.0, seed).astype(np.float32 if dt == F32 else np.float64)


def _dot(a, b):
    return sum(float((x.double() * y.double()).sum()) for x, y in zip(a, b))


def _norm(a):
    return float(torch.sqrt(sum((x.double() ** 2).sum() for x in a)))


@pytest.mark.parametrize("direction", ["build", "reconstruct", "build_adjoint", "reconstruct_adjoint"])
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cfg", SCF_CONFIGS, ids=lambda c: "%d-%d-%d" % c)
def test_scfpyr_memory_contract(scf, oracle, dev, cfg, n, precision, direction):
    """Bounds.  build: the oracle call and bound of test_scfpyr_large_side_vs_oracle.  reconstruct, precision 64: 1e-12 relative, as
    test_scfpyr_reconstruct_gpu.py; precision 32 there is bounded by a per-geometry figure of the golden fixture, which has no
    97-pixel geometry, so here: float64 inside and ONE rounding of each output element to fp32 -- 2^-24 of the largest magnitude --
    on top of the float64 bound.  Adjoints: the dot-product identity at the 1e-12 relative bound of test_build_adjoint_identity,
    with the forward side evaluated by the library at precision 64 (checked against its own references above); at precision
    32 the adjoint's output is rounded once, which moves <x, A^T w> by at most 2^-24 |x| |A^T w| (Cauchy-Schwarz), added to the
    bound."""
    from mimamo_net_amd.scfpyr import SCFpyr_PyTorch
    L = _lib.lib()
    size, height, nbands = cfg
    h, shapes = scf(size, height, nbands, n)
    dt = F32 if precision == 32 else F64
    to_coeffs = direction in ("build", "reconstruct_adjoint")      # image -> coefficients, else coefficients -> image
    image = _scf_rand("mc.scf.img", (n, size, size), size, dt)
    if direction == "build":
        image = (image + 1) / 2                                    # [0, 1) as the oracle-backed build tests use; still exact in fp32
    coeffs = [_scf_rand("mc.scf.c%d" % k, shp, size + 1, dt) for k, shp in enumerate(shapes)]
    need = L.mm_scfpyr_workspace_bytes(h, n)
    fn = getattr(L, "mm_scfpyr_" + direction)
    if to_coeffs:
        src = [guarded(image.shape, dt, dev, image)]
    else:
        src = [guarded(c.shape, dt, dev, c) for c in coeffs]
    src_ptrs = (ctypes.c_void_p * len(src))(*[t.data_ptr() for t, _ in src])

    def run(ws_ptr, ws_bytes, dst):
        dst_ptrs = (ctypes.c_void_p * len(dst))(*[t.data_ptr() for t, _ in dst])
        if to_coeffs:
            return fn(h, src_ptrs[0], precision, n, dst_ptrs, ws_ptr, ws_bytes, _lib.current_stream())
        return fn(h, src_ptrs, precision, n, dst_ptrs[0], ws_ptr, ws_bytes, _lib.current_stream())

    def outputs():
        return [guarded(s, dt, dev, SENTINEL) for s in (shapes if to_coeffs else [(n, size, size)])]
    outs = {}
    for fname, fill in FILLS.items():
        dst = outputs()
        ws, ckw = _workspace(need, dev, fill, F64)
        rc = run(_lib.ptr(ws), need, dst)
        torch.cuda.synchronize()
        assert rc == _lib.MM_OK, (fname, rc)
        ckw("workspace (%s)" % fname)
        for k, (t, ck) in enumerate(src):
            ck("input %d" % k)
        for k, (t, ck) in enumerate(dst):
            ck("output %d" % k)
            assert_fully_written(t)
        outs[fname] = [t.clone() for t, _ in dst]
    for (t, _), a in zip(src, [image] if to_coeffs else coeffs):
        assert torch.equal(t, torch.from_numpy(a).to(dev))
    _same_across_fills(outs, direction)
    got = outs["nan"]
    eps32 = 2.0 ** -24 if precision == 32 else 0.0
    if direction == "build":
        levels, hi, lo = oracle.pyramid_build(image.astype(np.float64), height, nbands, dtype=np.float64, keep_residuals=True)
        want = [hi] + [np.stack([c[b].real, c[b].imag], -1) for c in levels for b in range(nbands)] + [lo]
        tol = 3e-7 if precision == 32 else 1e-12
        for k, (g, w) in enumerate(zip(got, want)):
            assert tuple(g.shape) == w.shape
            err = np.abs(g.double().cpu().numpy() - w).max()
            assert err <= tol * max(1.0, np.abs(w).max()), (k, err)
    elif direction == "reconstruct":
        want = _host_reconstruct(coeffs, size, height, nbands)
        err = np.abs(got[0].double().cpu().numpy() - want).max()
        scale = max(1.0, np.abs(want).max())
        print("reconstruct %s n %d precision %d: max err %.2e (|want| max %.2e)" % (cfg, n, precision, err, np.abs(want).max()))
        assert err <= (1e-12 + eps32) * scale, err
    else:
        pyr = SCFpyr_PyTorch(height=height, nbands=nbands, scale_factor=2, device=dev, precision=64)
        x = torch.from_numpy(image.astype(np.float64)).to(dev)
        cs = [torch.from_numpy(c.astype(np.float64)).to(dev) for c in coeffs]
        if direction == "build_adjoint":          # <build(x), w> == <x, build^T w>
            fwd = pyr.build(x[:, None])
            flat = [fwd[0]] + [b for lvl in fwd[1:-1] for b in lvl] + [fwd[-1]]
            lhs, rhs = _dot(flat, cs), _dot([x], got)
            bound = (1e-12 + eps32) * _norm([x]) * _norm(got)
        else:                                     # <reconstruct(c), y> == <c, reconstruct^T y>
            nest = [cs[0]] + [cs[1 + l * nbands:1 + (l + 1) * nbands] for l in range(height - 2)] + [cs[-1]]
            lhs, rhs = _dot([pyr.reconstruct(nest)], [x]), _dot(cs, got)
            bound = (1e-12 + eps32) * _norm(cs) * _norm(got)
        pyr.close()
        print("%s %s n %d precision %d: |lhs - rhs| %.2e, bound %.2e" % (direction, cfg, n, precision, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    dst = outputs()
    _refused(lambda w, b: run(w, b, dst), need, dev, dst, F64)


# ======================================================================================================================
# Stale cached workspaces through the Python classes
# ======================================================================================================================
STALE = [(k, v) for k, v in FILLS.items() if k != "zeros"]


def _stream_key():
    return torch.cuda.current_stream().cuda_stream


def test_resnet50_extractor_ignores_a_stale_cached_workspace(pkg, dev):
    from mimamo_net_amd.resnet50_extractor import Resnet50_Extractor
    sd = weights.make_resnet50_state_dict(seed=0)
    x = torch.from_numpy(_images(5, 31)).to(dev)
    small = x[:2].contiguous()
    fresh = Resnet50_Extractor(state_dict=sd, device=dev)
    want = fresh.get_vec(small).clone()
    fresh.close()
    ext = Resnet50_Extractor(state_dict=sd, device=dev)
    ext.get_vec(x)                                       # the larger call sizes the cached workspace
    assert torch.equal(ext.get_vec(small), want)         # ... and leaves its activations there
    ws = ext._ws[_stream_key()]
    assert ws.numel() * 4 >= _lib.lib().mm_resnet50_workspace_bytes(ext._handle, 5)
    for name, fill in STALE:
        ws.fill_(fill)
        got = ext.get_vec(small)
        assert ext._ws[_stream_key()] is ws
        assert torch.isfinite(got).all() and torch.equal(got, want), name
    ext.close()


def test_two_stream_rnn_ignores_a_stale_cached_workspace(pkg, dev):
    from mimamo_net_amd.mimamo_net import Two_Stream_RNN
    sd = weights.make_two_stream_state_dict(seed=3)
    t = lambda name, shape, lo, hi: torch.from_numpy(weights.det_uniform(name, shape, lo, hi, 50)).to(dev)
    big = (t("mc.st.p0", (3, 8, 24, 48, 48), -1.5, 1.5), t("mc.st.p1", (3, 8, 24, 24, 24), -1.5, 1.5), t("mc.st.rgb", (3, 8, 2048), 0.0, 2.0))
    small = tuple(a[:2, :3].contiguous() for a in big)
    want = Two_Stream_RNN().load_state_dict(sd).eval().to(dev)([small[0], small[1]], small[2]).clone()
    m = Two_Stream_RNN().load_state_dict(sd).eval().to(dev)
    m([big[0], big[1]], big[2])
    assert torch.equal(m([small[0], small[1]], small[2]), want)
    ws = m._ws[_stream_key()]
    for name, fill in STALE:
        ws.fill_(fill)
        got = m([small[0], small[1]], small[2])
        assert m._ws[_stream_key()] is ws
        assert torch.isfinite(got).all() and torch.equal(got, want), name


def test_phase_difference_extractor_ignores_a_stale_cached_workspace(pkg, dev):
    from mimamo_net_amd.phase_difference_extractor import Phase_Difference_Extractor
    frames = torch.from_numpy(synthetic.textured_gray(64, 48, seed=300)).to(dev)
    small = frames[:20].contiguous()
    ids_big, ids_small = _clip_windows(0, 64, dev), _clip_windows(0, 20, dev)
    kw = dict(nhwc=True, out1_cstride=88, out1_coffset=64)
    fresh = Phase_Difference_Extractor(4, 2, 2, [1, 2], False)
    w0, w1 = fresh.phase_diff_frames(small, ids_small, **kw)
    w0, w1 = w0.clone(), w1[..., 64:].clone()
    pde = Phase_Difference_Extractor(4, 2, 2, [1, 2], False)
    pde.phase_diff_frames(frames, ids_big, **kw)
    ws = pde._ws[_stream_key()]
    for name, fill in [("after the larger call", None)] + STALE:
        if fill is not None:
            ws.fill_(fill)
        g0, g1 = pde.phase_diff_frames(small, ids_small, **kw)
        assert pde._ws[_stream_key()] is ws
        assert torch.isfinite(g0).all() and torch.equal(g0, w0) and torch.equal(g1[..., 64:], w1), name
