"""Self-test of tests/poison.py (no GPU: the guard-banded path is exercised on CPU blocks)."""
import numpy as np
import pytest
import torch

from tests.poison import PATTERNS, equals_pattern, poisoned_allocations


def _alloc_here(n):
    return torch.empty(n, dtype=torch.float64)          # the call site the report must name


@pytest.mark.parametrize("pattern", PATTERNS)
def test_views_have_the_requested_dtype_shape_and_pattern(pattern):
    with poisoned_allocations(pattern, devices=("cpu",)) as st:
        a = torch.empty(3, 5, dtype=torch.float32)
        b = torch.empty((7,), dtype=torch.int32)
        c = torch.empty_like(a, dtype=torch.float64)
        d = a.new_empty((2, 2), dtype=torch.uint8)
        e = torch.empty_strided((4, 3), (3, 1), dtype=torch.int64)
        f = torch.empty(size=(2, 3), dtype=torch.bool)
        for t, shape, dt in ((a, (3, 5), torch.float32), (b, (7,), torch.int32), (c, (3, 5), torch.float64),
                             (d, (2, 2), torch.uint8), (e, (4, 3), torch.int64), (f, (2, 3), torch.bool)):
            assert t.shape == shape and t.dtype == dt and t.is_contiguous()
            assert equals_pattern(t.numpy(), pattern).all()
        assert len(st.blocks) == 6
        assert all(blk.base.numel() == blk.nbytes + 2 * 4096 for blk in st.blocks)
        # the returned view starts `guard` bytes into its block (vector-load alignment kept)
        assert all(int(t.untyped_storage().data_ptr()) + 4096 == t.data_ptr() for t in (a, b, c))
        # non-contiguous and zero-byte requests: no guard band, still filled
        g = torch.empty_like(torch.zeros(4, 6).t())
        z = torch.empty(0, 3)
        assert len(st.blocks) == 6 and z.numel() == 0
        assert equals_pattern(g.contiguous().numpy(), pattern).all()
    # the pattern the helper documents
    if pattern == 0xFF:
        assert np.isnan(a.numpy()).all() and np.isnan(c.numpy()).all() and (b.numpy() == -1).all()
    if pattern == 0x7F:
        assert (c.numpy() > 1e306).all() and (a.numpy() > 3e38).all() and (b.numpy() == 0x7F7F7F7F).all()


def test_constructors_with_defined_content_are_untouched():
    with poisoned_allocations(0xFF, devices=("cpu",)) as st:
        z, o = torch.zeros(5, dtype=torch.float64), torch.full((3,), 2.5)
        assert (z.numpy() == 0).all() and (o.numpy() == 2.5).all() and not st.blocks


@pytest.mark.parametrize("where", ["after", "before"])
def test_a_write_into_a_guard_names_the_call_site(where):
    with pytest.raises(AssertionError) as err:
        with poisoned_allocations(0x7F, devices=("cpu",)) as st:
            x = _alloc_here(10)
            torch.empty(3, dtype=torch.int32)
            x.fill_(1.0)                                 # inside the buffer: fine
            st.check_guards()
            base = st.blocks[0].base
            if where == "after":
                base[4096 + 80 + 3] = 0                  # the fourth byte past the last element
            else:
                base[4096 - 16] = 0
    msg = str(err.value)
    assert "test_poison_helper.py" in msg and "_alloc_here" in msg
    assert "80-byte buffer" in msg and f"guard byte {where}" in msg
    assert ("offset 83" in msg) if where == "after" else ("offset -16" in msg)
    assert msg.count("buffer (") == 1                    # the intact neighbour is not reported


def test_nothing_outside_the_context_is_affected():
    orig = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with poisoned_allocations(0xFF, devices=("cpu",)):
        assert torch.empty is not orig[0]
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == orig
    with pytest.raises(RuntimeError):
        with poisoned_allocations(0xFF, devices=("cpu",)):
            raise RuntimeError("body fails")
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == orig
    a = torch.empty(1000, dtype=torch.float64)
    assert a.shape == (1000,) and a.untyped_storage().nbytes() == 8000
