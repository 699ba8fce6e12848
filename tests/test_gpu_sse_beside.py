"""Beside mode (MF_SSE_BESIDE=1): sse_async() snapshots the parameters, and the
pass runs on a side stream beside the NEXT epoch's persistent sweep, released
by that launch's resident ticket (or, at the latest, by the write behind the
sweep).  The sweep waits on nothing new, so the parameters must be the same
bits with the mode on and off; a slot's pass runs with one workgroup per CU
whichever way it is released, so it must be the same bits as a serial
sse_from(max_blocks=CUs) on the parameters saved after that epoch, and within
1e-12 relative of the default pass (only the grouping of the per-workgroup
partial sums differs; the sum has ~6e4 terms of FP64).

Shape: the smallest that takes the stream kernel with 4 user-range classes
(B = 8 workgroups, 32 strata), as in test_gpu_strata's stream cases.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NU, NI, NNZ, B, C = 4096, 512, 60000, 8, 4
EPOCHS = 5


def _data():
    rs = np.random.RandomState(31)
    keys = rs.choice(NU * NI, NNZ, replace=False)
    u = (keys // NI).astype(np.int32)
    i = (keys % NI).astype(np.int32)
    r = rs.randint(1, 6, NNZ).astype(np.float64)
    return u, i, r


def _engine(dtype, kernel, k, waves=None):
    from matrix_factorization.engine import SGDEngine

    u, i, r = _data()
    rs = np.random.RandomState(32)
    eng = SGDEngine(u, i, r, NU, NI, k, kernel, dtype, "cuda:0", gamma=1.0 / k, min_rating=1.0,
                    max_rating=5.0, global_mean=float(r.mean()))
    eng.load_params(rs.normal(0, 0.1, (NU, k)), rs.normal(0, 0.1, (NI, k)),
                    rs.normal(0, 0.1, NU), rs.normal(0, 0.1, NI))
    eng.prepare_strata(n_blocks=B, classes=C, waves=waves)
    return eng


def _run(monkeypatch, beside, dtype, kernel, k, epochs=EPOCHS, waves=None):
    """(engine, parameters saved after every epoch, SSE slots, was the mode on)."""
    from matrix_factorization.engine import stratum_order

    monkeypatch.setenv("MF_STRATA_DEEP", "1")
    monkeypatch.setenv("MF_SSE_BESIDE", "1" if beside else "0")
    eng = _engine(dtype, kernel, k, waves)
    active = eng.beside_active
    saved = []
    for ep in range(epochs):
        seq = stratum_order(np.random.RandomState(ep), eng.strata)
        eng.epoch_strata(seq, 7000 + ep, lr=0.01, reg=0.02)
        eng.sse_async(ep)
        saved.append(eng.snapshot_params())
    sse = eng.sse_values(epochs)
    eng.check_strata()
    return eng, saved, sse, active


def _serial_capped(eng, saved):
    """sse_from(max_blocks=CUs) on each saved parameter set, on the launch stream."""
    import torch

    main = torch.cuda.current_stream(eng.dev)
    ws = torch.empty_like(eng.ws)
    for ep, snap in enumerate(saved):
        eng.sse_from(100 + ep, *snap, ws, main, max_blocks=eng._cus())
    torch.cuda.synchronize()
    return eng.sse_buf[100:100 + len(saved)].cpu().numpy()


def _same_params(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kernel,k", [("linear", 64), ("sigmoid", 64), ("linear", 8),
                                      ("sigmoid", 8)])
def test_beside_equals_serial(monkeypatch, kernel, k):
    from matrix_factorization import _lib

    on, saved, sse_on, active = _run(monkeypatch, True, "float64", kernel, k)
    if k == 64:
        # the FP64 rank-64 stream kernel leaves room for exactly one pass workgroup
        assert active, on.beside_info
        sub = on.strata.phases[0] if hasattr(on.strata, "phases") else on.strata
        assert on._strata_flags(sub, None) & _lib.MF_FLAG_STREAM
    off, _, sse_off, was_off = _run(monkeypatch, False, "float64", kernel, k)
    assert not was_off
    _same_params(on.params_numpy(), off.params_numpy())
    if active:
        assert np.array_equal(sse_on, _serial_capped(on, saved))
    else:
        assert np.array_equal(sse_on, sse_off)
    print("sse on/off max rel diff", np.max(np.abs(sse_on - sse_off) / sse_off))
    assert np.all(np.abs(sse_on - sse_off) <= 1e-12 * sse_off)


def test_flush_paths(monkeypatch):
    """A pending pass with no sweep behind it runs alone: at rmse_values(),
    and at a second sse_async()."""
    eng, saved, sse, active = _run(monkeypatch, True, "float64", "linear", 64, epochs=1)
    assert active
    ref = _serial_capped(eng, saved)
    assert np.array_equal(sse, ref)                  # sse_async -> sse_values
    eng.sse_async(1)
    eng.sse_async(2)                                 # flushes slot 1's pending pass
    assert eng._bs["pending"] == 2
    got = eng.sse_values(3)
    assert np.array_equal(got, np.repeat(ref, 3))
    assert eng._bs["pending"] is None
    assert eng.rmse_values(1)[0] == float(np.sqrt(ref[0] / NNZ))


def test_per_stratum_epochs_complete_through_the_backstop(monkeypatch):
    """MF_STRATA_PERSISTENT=0: no launch of the epoch stores a ticket; the
    write behind the epoch's launches releases the pass."""
    ref_eng, _, sse_ref, _ = _run(monkeypatch, False, "float64", "linear", 64)
    monkeypatch.setenv("MF_STRATA_PERSISTENT", "0")
    eng, saved, sse, active = _run(monkeypatch, True, "float64", "linear", 64)
    assert active
    _same_params(eng.params_numpy(), ref_eng.params_numpy())
    assert np.array_equal(sse, _serial_capped(eng, saved))
    assert np.all(np.abs(sse - sse_ref) <= 1e-12 * sse_ref)


def test_fp32_rank64_stays_as_it_is(monkeypatch):
    """The FP32 rank-64 sweep (16 waves of 128 registers, C3's form) fills
    the register file: the fit check says no, the engine reports the mode
    inactive and runs today's pass."""
    on, _, sse_on, active = _run(monkeypatch, True, "float32", "linear", 64, waves=16)
    assert not active and not on.beside_active, on.beside_info
    off, _, sse_off, _ = _run(monkeypatch, False, "float32", "linear", 64, waves=16)
    assert np.array_equal(sse_on, sse_off)
    _same_params(on.params_numpy(), off.params_numpy())
