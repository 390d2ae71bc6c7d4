"""The guards of tests/kernel_harness.py themselves, on the GPU: every kernel test relies on ``Buf`` and ``ByteBuf``
noticing a write one element outside the data, so that is pinned here.  No kernel is launched - the stray writes are
torch writes through ``whole``, inside the allocation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_harness import GUARD_BYTES, Buf, ByteBuf, nan_out, poisoned  # noqa: E402

pytestmark = pytest.mark.gpu
N = 5


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("where", ["before", "after"])
def test_a_word_next_to_the_data_of_a_buf_is_a_guard(offset, where):
    """One word before and one word after the data, aligned and with ptr % 16 == 4."""
    b = Buf(np.arange(N, dtype=np.float32), offset)
    assert b.ptr % 16 == 4 * offset and b.ptr == b.whole.data_ptr() + 4 * b.start
    b.check_guards("untouched")
    b.whole[b.start:b.start + N] = 7                             # the data itself is no guard
    b.check_guards("data written")
    b.whole[b.start - 1 if where == "before" else b.start + N] = 0
    with pytest.raises(AssertionError, match="a guard word was written"):
        b.check_guards(where)


@pytest.mark.parametrize("where", ["before", "after"])
def test_a_byte_next_to_the_data_of_a_bytebuf_is_a_guard(where):
    b = ByteBuf(N)
    assert b.ptr == b.whole.data_ptr() + GUARD_BYTES and b.ptr % 2 == 1
    b.check_guards("untouched")
    b.raw[:] = 3
    b.check_guards("data written")
    b.whole[GUARD_BYTES - 1 if where == "before" else GUARD_BYTES + N] = 0
    with pytest.raises(AssertionError, match="a guard byte was written"):
        b.check_guards(where)


def test_a_fresh_output_is_poisoned_until_written():
    b = nan_out(N)
    assert b.get().shape == (N,) and poisoned(b.get()).all()
    b.t[3] = 1.5
    assert poisoned(b.get()).tolist() == [True, True, True, False, True]
    b.check_guards("one element written")


def test_an_empty_buf_has_no_pointer():
    b = Buf(np.zeros(0, np.float32))
    assert b.ptr is None and b.get().shape == (0,)
    b.check_guards("empty")
