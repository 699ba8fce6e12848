"""Host-side parts of matrix_factorization.device_model (no device): the two
CSR normalisers against per-query Python restatements, and the module split
itself (SGDEngine is a DeviceModel; engine.py still exports every moved name)."""

import numpy as np
import pytest

from matrix_factorization.device_model import DeviceModel, exclusion_csr, target_csr


def lists_of(n_query, seed):
    """Per-query item lists of length 0 to 5, unsorted, with repeats."""
    rs = np.random.RandomState(seed)
    return [rs.randint(-2, 90, rs.randint(0, 6)).tolist() for _ in range(n_query)]


def flatten(lists, lead=(), trail=()):
    """(ptr, items): the lists as a CSR whose items array has ``lead`` before
    the first list (ptr starts at len(lead)) and ``trail`` after the last."""
    ptr = len(lead) + np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    items = np.asarray(list(lead) + [v for x in lists for v in x] + list(trail), np.int32)
    return ptr, items


def restated(ptr, items, sort):
    """Slice each query's list, optionally sorted(), concatenate."""
    per = [items[ptr[q]:ptr[q + 1]].tolist() for q in range(len(ptr) - 1)]
    per = [sorted(x) if sort else x for x in per]
    flat = [v for x in per for v in x]
    want_ptr = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int64)
    return want_ptr, np.asarray(flat if flat else [0], np.int32)


LAYOUTS = {"from_zero": ((), ()), "offset_3": ((97, 98, 99), ()), "trailing": ((), (95, 96)),
           "offset_and_trailing": ((97, 98, 99), (95, 96))}
# n_query 0, 1 and 7 with random lists of 0..5 items, and 7 all-empty lists
LISTS = {"nq0": [], "nq1": lists_of(1, 1), "nq7": lists_of(7, 2), "nq7_empty": [[]] * 7,
         "nq1_len5": [[9, 3, 3, -1, 50]]}


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("lists", sorted(LISTS))
def test_exclusion_csr_matches_the_restatement(lists, layout, sort):
    lists = LISTS[lists]
    ptr, items = flatten(lists, *LAYOUTS[layout])
    got_ptr, got_items = exclusion_csr(len(lists), ptr, items, sort)
    want_ptr, want_items = restated(ptr, items, sort)
    assert got_ptr.dtype == np.int64 and got_items.dtype == np.int32
    assert np.array_equal(got_ptr, want_ptr) and got_ptr[0] == 0
    assert np.array_equal(got_items, want_items)
    assert len(got_items) >= 1                           # the dummy: never an empty array


def test_exclusion_csr_cases_hold_empty_and_longest_lists():
    lengths = {len(x) for case in LISTS.values() for x in case}
    assert {0, 5} <= lengths <= set(range(6))
    assert 0 in {len(x) for x in LISTS["nq7"]} and max(len(x) for x in LISTS["nq7"]) > 1


@pytest.mark.parametrize("sort", [True, False])
def test_exclusion_csr_accepts_other_integer_types(sort):
    ptr, items = flatten(LISTS["nq7"], (97, 98, 99))
    a = exclusion_csr(7, ptr.astype(np.int32).tolist(), items.astype(np.int64), sort)
    b = exclusion_csr(7, ptr, items, sort)
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


@pytest.mark.parametrize("sort", [True, False])
def test_exclusion_csr_without_exclusions(sort):
    assert exclusion_csr(7, None, None, sort) == (None, None)
    assert exclusion_csr(0, None, np.zeros(3, np.int32), sort) == (None, None)


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("n_query", [0, 1, 7])
def test_exclusion_csr_refuses_a_wrong_length(n_query, sort):
    for n in (n_query, n_query + 2):
        with pytest.raises(ValueError, match=r"ex_ptr needs n_query \+ 1 offsets"):
            exclusion_csr(n_query, np.zeros(n, np.int64), np.zeros(4, np.int32), sort)


def test_target_csr():
    lists = lists_of(7, 3)
    ptr, items = flatten(lists)
    got_ptr, got_items, nt = target_csr(7, ptr, items)
    assert got_ptr.dtype == np.int64 and got_items.dtype == np.int32
    assert np.array_equal(got_ptr, ptr) and np.array_equal(got_items, items) and nt == len(items)
    # targets keep their order: nothing is sorted
    assert got_items.tolist() == [v for x in lists for v in x]
    # items beyond the last offset are cut
    _, cut, nt2 = target_csr(7, ptr, np.concatenate([items, [5, 6]]))
    assert nt2 == nt and np.array_equal(cut, items)
    # a rebased ptr gives its zero-based form's output (the items are NOT
    # sliced from ptr[0]: the kernels' contract is offsets relative to the
    # first, into an array that starts with the first target)
    for a, b in zip(target_csr(7, ptr + 11, items), (got_ptr, got_items, nt)):
        assert np.array_equal(a, b)


def test_target_csr_refuses_bad_offsets():
    items = np.arange(6, dtype=np.int32)
    with pytest.raises(ValueError, match="tgt_ptr must be non-decreasing and end within"):
        target_csr(3, [0, 4, 2, 6], items)                       # decreasing
    with pytest.raises(ValueError, match="tgt_ptr must be non-decreasing and end within"):
        target_csr(3, [0, 2, 4, 7], items)                       # ends past tgt_items
    with pytest.raises(ValueError, match="tgt_ptr must be non-decreasing and end within"):
        target_csr(3, [5, 7, 9, 12], items)                      # ... after rebasing too
    for n in (3, 5):
        with pytest.raises(ValueError, match=r"tgt_ptr needs n_query \+ 1 offsets"):
            target_csr(3, np.zeros(n, np.int64), items)
    with pytest.raises(ValueError, match=r"tgt_ptr needs n_query \+ 1 offsets"):
        target_csr(0, np.zeros(0, np.int64), items)


def test_target_csr_without_queries():
    ptr, items, nt = target_csr(0, np.array([4]), np.arange(9, dtype=np.int32))
    assert ptr.tolist() == [0] and len(items) == 0 and nt == 0
    ptr, items, nt = target_csr(0, np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert ptr.tolist() == [0] and len(items) == 0 and nt == 0


MOVED = ("_VOID", "DTYPES", "canonical_dtype", "resolve_device", "_WARMED", "_warm_device",
         "_under_rocprofiler", "_tp", "_np", "_HipBlock", "_contiguous_empty")
SERVING = ("stream", "_dev", "_dev_rows", "load_params", "params_numpy", "predict",
           "topk_ws_budget", "topk_mfma", "topk_prepare", "_topk_workspace", "topk_launch",
           "topk_finish", "topk", "rank_ws_budget", "rank", "_model_args")


def test_engine_is_a_device_model_and_still_exports_the_moved_names():
    from matrix_factorization import device_model, engine

    assert DeviceModel in engine.SGDEngine.__mro__[1:]
    assert engine.DeviceModel is DeviceModel
    for name in MOVED:
        assert getattr(engine, name) is getattr(device_model, name), name
    # the serving half is inherited, not restated or forwarded
    for name in SERVING:
        assert name in vars(DeviceModel), name
        assert name not in vars(engine.SGDEngine), name
    assert engine.SGDEngine.topk_ws_budget == DeviceModel.topk_ws_budget == 1 << 30
