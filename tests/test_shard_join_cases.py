"""The join of tests/shard_threads.py alone (no GPU): the element-wise unsigned minimum that the threads of
tests/test_gpu_row_shard_classes.py put in the place of the all-reduce, on buffers of both element widths the engine
hands out (32-bit level-1 / hetcor marks, 64-bit selection ranks)."""
import numpy as np
import pytest

from shard_threads import join_buffers, unsigned_min

WIDTHS = [(4, np.uint32, np.int32), (8, np.uint64, np.int64)]
IDS = ["32bit", "64bit"]


def _none(udt):
    return udt(np.iinfo(udt).max)


@pytest.mark.parametrize("elem,udt,sdt", WIDTHS, ids=IDS)
def test_none_loses_to_every_value(elem, udt, sdt):
    none, top = _none(udt), int(np.iinfo(udt).max)
    values = np.array([0, 1, 2, 1 << (8 * elem - 1), (1 << (8 * elem - 1)) - 1, top - 1, top], udt)
    a = np.full(values.size, none, udt)
    for bufs in ([a, values], [values, a]):
        out = unsigned_min(bufs, elem)
        assert out.dtype == udt and np.array_equal(out, values)
    assert np.array_equal(unsigned_min([a, a], elem), a)  # nobody found anything: still none


@pytest.mark.parametrize("elem,udt,sdt", WIDTHS, ids=IDS)
def test_top_bit_values_compare_as_unsigned(elem, udt, sdt):
    """the engine's buffers reach Python as signed views as often as not (torch has no uint64): the join must not care"""
    hi = 1 << (8 * elem - 1)
    big = np.array([hi, hi + 5, hi | 1, int(np.iinfo(udt).max)], udt)
    small = np.array([hi - 1, 7, 0, hi], udt)
    want = np.array([hi - 1, 7, 0, hi], udt)
    assert np.array_equal(unsigned_min([big, small], elem), want)
    # the same bytes handed over as signed integers: a signed minimum would pick the negative (= large unsigned) ones
    assert (big.view(sdt) < 0).all()
    assert np.array_equal(unsigned_min([big.view(sdt), small.view(sdt)], elem), want)
    assert not np.array_equal(np.minimum(big.view(sdt), small.view(sdt)).view(udt), want)
    # both with the top bit set: the smaller unsigned value
    both = unsigned_min([np.array([hi + 9], udt).view(sdt), np.array([hi + 3], udt).view(sdt)], elem)
    assert both.tolist() == [hi + 3]


@pytest.mark.parametrize("elem,udt,sdt", WIDTHS, ids=IDS)
def test_three_buffers_one_all_none(elem, udt, sdt):
    rng = np.random.default_rng(elem)
    top = int(np.iinfo(udt).max)
    a = rng.integers(0, top, 257, dtype=udt, endpoint=True)
    b = rng.integers(0, top, 257, dtype=udt, endpoint=True)
    a[::7] = _none(udt)  # none on one side, on both (every 35th), on neither
    b[::5] = _none(udt)
    idle = np.full(257, _none(udt), udt)  # a rank that owns no row with work
    want = np.where(a < b, a, b)
    for bufs in ([a, b, idle], [idle, a, b], [a, idle, b]):
        assert np.array_equal(unsigned_min(bufs, elem), want)
    assert (want[::35] == _none(udt)).all() and (want != _none(udt)).sum() > 150


@pytest.mark.parametrize("elem,udt,sdt", WIDTHS, ids=IDS)
def test_result_is_written_to_every_participant(elem, udt, sdt):
    rng = np.random.default_rng(10 + elem)
    top = int(np.iinfo(udt).max)
    bufs = [rng.integers(0, top, 64, dtype=udt, endpoint=True) for _ in range(5)]
    bufs[3] = bufs[3].view(sdt)  # (a signed view is written through as well)
    want = np.minimum.reduce([b.view(udt) for b in bufs])
    copies = [b.copy() for b in bufs]
    out = join_buffers(bufs, elem)
    assert np.array_equal(out, want)
    for b, c in zip(bufs, copies):
        assert np.array_equal(b.view(udt), want)
        assert not np.array_equal(c.view(udt), want)  # (no participant held the minimum everywhere beforehand)
    # one participant, and empty buffers (a graph without edges): unchanged, no error
    one = np.array([3, top], udt)
    assert np.array_equal(join_buffers([one], elem), [3, top]) and one.tolist() == [3, top]
    assert join_buffers([np.empty(0, udt), np.empty(0, udt)], elem).size == 0


def test_width_and_length_are_checked():
    with pytest.raises(ValueError):
        unsigned_min([np.zeros(4, np.uint16)], 2)
    with pytest.raises(ValueError):
        unsigned_min([np.zeros(4, np.uint32), np.zeros(5, np.uint32)], 4)
