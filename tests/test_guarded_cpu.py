"""The guard helper of the memory-contract tests (guarded.py) on host tensors: it must notice a one-element overrun on either
side, an element a call never wrote and an element outside the declared channel window that it did write -- and stay quiet otherwise."""
import pytest
import torch

import guarded as g

CPU = torch.device("cpu")


def _payload_end(t):
    return g.GUARD_BYTES + t.numel() * t.element_size()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_guards_are_nans_of_both_widths_and_the_payload_keeps_its_fill(dtype):
    for name, fill in g.FILLS.items():
        t, check = g.guarded((3, 5), dtype, CPU, fill)
        check()
        assert t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == (3, 5)
        assert torch.isnan(t).all() if name == "nan" else bool((t == torch.tensor(fill, dtype=dtype)).all())
        for lo in (0, _payload_end(t)):                       # (the guard above an fp32 payload need not be 8-byte aligned: clone first)
            guard = check.raw[lo:lo + g.GUARD_BYTES].clone()
            assert torch.isnan(guard.view(torch.float32)).all() and torch.isnan(guard.view(torch.float64)).all()
    assert g.GUARD_BYTES % 4096 == 0 and g.GUARD_BYTES >= 256 * 2048 * 4 and len(g.FILLS) == 4


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32, torch.uint8])
def test_one_element_past_either_end_is_noticed(dtype):
    src = torch.arange(7, dtype=dtype)
    for offset in (-1, 0):       # the last byte of the guard below, the first byte of the guard above
        t, check = g.guarded((7,), dtype, CPU, src)
        check()
        assert torch.equal(t, src)
        at = g.GUARD_BYTES + offset if offset < 0 else _payload_end(t)
        check.raw[at] = 0
        with pytest.raises(AssertionError, match="ABOVE|BELOW|behind"):
            check()
    t, check = g.guarded((7,), dtype, CPU, src)
    check.raw[-1] = 0                                        # and the far end of the guard above
    with pytest.raises(AssertionError, match="ABOVE"):
        check()
    if dtype in (torch.uint8, torch.int32):                  # integer payloads: 0xFF bytes / 0x7fffffff
        word = check.raw[:4].view(torch.int32).item()
        assert word == (-1 if dtype == torch.uint8 else 0x7FFFFFFF)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_unwritten_and_stray_output_elements_are_noticed(dtype):
    t, check = g.guarded((4, 6, 88), dtype, CPU, g.SENTINEL)
    g.assert_untouched(t)
    with pytest.raises(AssertionError, match="never written"):
        g.assert_fully_written(t)
    t[..., 64:88] = 0.5
    g.assert_fully_written(t, (64, 88))
    g.assert_untouched(t, (64, 88))
    t[3, 5, 87] = torch.nan                                  # an ordinary NaN is a written value, not the sentinel
    g.assert_fully_written(t, (64, 88))
    t[1, 2, 63] = 0.0
    with pytest.raises(AssertionError, match="outside the declared output window"):
        g.assert_untouched(t, (64, 88))
    check()
