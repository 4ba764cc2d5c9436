"""Guarded device buffers for the memory-contract tests (test_memory_contract_gpu.py): every buffer a native entry point
sees -- input, output, workspace -- sits between two guard regions that the test owns, so a store past a ragged tile or a
load of a neighbouring row lands in memory whose content is known, and can be told afterwards.

    payload, check = guarded(shape, dtype, dev, fill)

allocates ONE flat device buffer of `guard + payload + guard` bytes.  The guards hold a sentinel; `check()` asserts that both
are bit-for-bit what they were.  Guards are compared as int32 words, never as floats (the sentinel is a NaN: NaN != NaN).

Sentinels.  Floating-point guards repeat the 32-bit word 0x7ff8beef: alone it is a quiet fp32 NaN, and any two of them are
a quiet fp64 NaN (0x7ff8beef7ff8beef), so a kernel that LOADS from a guard gets a NaN whatever it reads it as.  Outputs are
pre-filled with a second NaN word (0x7ff8d00d): assert_fully_written() finds the elements a call left alone,
assert_untouched() checks the ones it had to leave alone.  uint8 guards hold 0xFF bytes, int32 guards 0x7fffffff.

FILLS is what a workspace (or an in/out buffer) holds before the call: zeros -- what a fresh allocator mostly hands out, the
lucky case -- a quiet NaN, and a large finite value of each sign: fmaxf / fminf, ReLU and a clamp swallow a NaN, +3e38
survives a max and -3e38 a min.
"""
import numpy as np
import torch

GUARD_BYTES = 1024 * 4096            # 4 MiB per side: more than one 256-row x 2048-channel fp32 tile (2 MiB); a multiple of 4096
assert GUARD_BYTES % 4096 == 0 and GUARD_BYTES >= 4 << 20

_GUARD_WORD = 0x7FF8BEEF            # a quiet NaN as fp32, and twice in a row (0x7ff8beef7ff8beef) as fp64
_OUT_WORD = 0x7FF8D00D              # the same for the output sentinel
_INT_GUARD = 0x7FFFFFFF

FILLS = {"zeros": 0.0, "nan": float("nan"), "+3e38": 3e38, "-3e38": -3e38}
SENTINEL = "sentinel"                # fill= of an output buffer

_patterns = {}


def _pattern(word, n_words, dev):
    """int32 [n_words] of one word (cached per device: the guards of every buffer compare against it)."""
    key = (word, n_words, str(dev))
    p = _patterns.get(key)
    if p is None:
        p = _patterns[key] = torch.full((n_words,), word, dtype=torch.int32, device=dev)
    return p


def _guard_word(dtype):
    if dtype == torch.uint8:
        return -1                                         # 0xFF bytes
    if dtype == torch.int32:
        return _INT_GUARD
    assert dtype in (torch.float32, torch.float64), dtype
    return _GUARD_WORD


def guarded(shape, dtype, dev, fill):
    """-> (payload, check).  payload: a contiguous `dtype` tensor of `shape` inside guard + payload + guard bytes; its address
    keeps the allocation's alignment (the guard is a multiple of 4096).  fill: a number (an entry of FILLS), SENTINEL (an
    output: the output NaN pattern), or an array / tensor of `shape` that is copied in.  check(): both guards intact."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = int(np.prod(shape)) * item if len(shape) else item
    pad = (-nbytes) % 4                                   # uint8 payloads only: the slack up to the guard's first int32 word
    raw = torch.empty((GUARD_BYTES + nbytes + pad + GUARD_BYTES,), dtype=torch.uint8, device=dev)
    pat = _pattern(_guard_word(dtype), GUARD_BYTES // 4, dev)
    lo = raw[:GUARD_BYTES].view(torch.int32)
    hi = raw[GUARD_BYTES + nbytes + pad:].view(torch.int32)
    slack = raw[GUARD_BYTES + nbytes:GUARD_BYTES + nbytes + pad]
    lo.copy_(pat)
    hi.copy_(pat)
    slack.fill_(0xFF)
    payload = raw[GUARD_BYTES:GUARD_BYTES + nbytes].view(dtype).view(shape)
    if isinstance(fill, str):
        assert fill == SENTINEL and dtype in (torch.float32, torch.float64)
        payload.view(-1).view(torch.int32).fill_(_OUT_WORD)
    elif isinstance(fill, (np.ndarray, torch.Tensor)):
        src = torch.from_numpy(np.ascontiguousarray(fill)) if isinstance(fill, np.ndarray) else fill
        assert tuple(src.shape) == shape and src.dtype == dtype, (tuple(src.shape), shape, src.dtype, dtype)
        payload.copy_(src)
    else:
        payload.fill_(fill)

    def check(what="buffer"):
        assert torch.equal(lo, pat), "%s: the guard BELOW it was written (%d words differ)" % (what, int((lo != pat).sum()))
        assert torch.equal(hi, pat), "%s: the guard ABOVE it was written (%d words differ, first at byte +%d)" % (
            what, int((hi != pat).sum()), 4 * int((hi != pat).int().argmax()))
        assert bool((slack == 0xFF).all()), "%s: the bytes right behind it were written" % what

    check.raw = raw                                       # keeps the allocation alive with the closure
    return payload, check


def _is_sentinel(t):
    """bool tensor: which elements of the fp32 / fp64 tensor t still hold the output sentinel (bit compare)."""
    if t.dtype == torch.float32:
        return t.view(torch.int32) == _OUT_WORD
    assert t.dtype == torch.float64
    return t.view(torch.int64) == (_OUT_WORD << 32 | _OUT_WORD)


def assert_fully_written(t, window=None):
    """No element of the output t (window=(lo, hi): of its channels [lo, hi), the last dimension) still holds the output
    sentinel it was pre-filled with."""
    if window is not None:
        t = t[..., window[0]:window[1]]
    left = int(_is_sentinel(t).sum())
    assert left == 0, "%d of %d output elements were never written" % (left, t.numel())


def assert_untouched(t, window=None):
    """Every element of t (window=(lo, hi): every channel OUTSIDE [lo, hi) of every row) still holds the output sentinel."""
    if window is None:
        parts = [t]
    else:
        parts = [t[..., :window[0]], t[..., window[1]:]]
    for p in parts:
        if p.numel():
            hit = int((~_is_sentinel(p)).sum())
            assert hit == 0, "%d elements outside the declared output window were written" % hit
