"""A factor model resident on one GPU: what scoring needs, and no more.

``DeviceModel`` holds the parameters (P, Q, b_u, b_i) as torch-ROCm tensors
with the kernel, dtype, gamma, rating bounds and global mean, and serves them
through libmf_hip.so: ``predict`` (mf_predict / mf_bias_predict), ``topk``
(mf_topk, mf_topk_mm) and ``rank`` (mf_rank).  It holds no ratings: the
estimators' predictors, the content-based cosine scoring and the hybrid
retrieval are DeviceModels, and ``engine.SGDEngine`` is a DeviceModel plus the
training state.

The host-side CSR handling of the query entry points lives here too
(``exclusion_csr``, ``target_csr``): the neighbourhood engine shares it.
"""

from __future__ import annotations

import ctypes
import os
import sys
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

_VOID = ctypes.c_void_p

DTYPES = {
    "float32": (torch.float32, np.float32, _lib.MF_F32),
    "float64": (torch.float64, np.float64, _lib.MF_F64),
}


def canonical_dtype(dtype) -> str:
    name = np.dtype(dtype).name
    if name not in DTYPES:
        raise ValueError(f"dtype must be float32 or float64, got {dtype!r}")
    return name


def resolve_device(device=None) -> torch.device:
    """The GPU the engine runs on.  There is no CPU path."""
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.MFLibraryError(
                "no HIP device visible: matrix_factorization trains on an "
                "AMD Instinct GPU (gfx950) through libmf_hip.so")
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device must be a HIP ('cuda') device, got {device!r}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _under_rocprofiler() -> bool:
    """True when rocprofv3's tool library is preloaded into this process
    (`rocprofv3 ... -- python ...` puts librocprofiler-sdk-tool in
    LD_PRELOAD).  Profiled runs then launch the persistent strata kernel
    plainly -- the same kernel; the occupancy check stays the co-residency
    guard -- and bench.py labels its line "launch": "plain (profiler)".
    Why ("the r05n abort"): one profiled top-k bench
    exited 139 in its C exit handlers after its JSON line was out; nothing
    ties that fault to the cooperative launch, so this is caution, kept
    narrow: only the preload counts, not any ROCPROF* variable in the
    environment (MF_PROFILER_PLAIN=0 turns it off)."""
    if os.environ.get("MF_PROFILER_PLAIN") == "0":
        return False
    return "librocprofiler" in os.environ.get("LD_PRELOAD", "")


_WARMED = set()


def _warm_device(dev: torch.device) -> None:
    """mf_warmup once per device and process: the runtime loads the library's
    code object at the first launch of any of its kernels -- done here, while
    an engine is built (fit() builds it on a worker thread beside the
    initial draws), instead of inside the first training epoch."""
    if dev.type != "cuda" or dev.index in _WARMED:
        return
    with torch.cuda.device(dev):
        # (no cooperative launch under rocprofv3: its interception crashes)
        _lib.call("mf_warmup", _lib.MF_FLAG_NO_COOP if _under_rocprofiler() else 0,
                  _VOID(torch.cuda.current_stream(dev).cuda_stream))
    _WARMED.add(dev.index)


def _tp(t: Optional[torch.Tensor]):
    if t is None or t.numel() == 0:
        return None
    return _VOID(t.data_ptr())


def _np(a: Optional[np.ndarray]):
    if a is None:
        return None
    return a.ctypes.data_as(_VOID)


class _HipBlock:
    """A physically contiguous device allocation, exposed to torch through
    __cuda_array_interface__ (torch keeps this object alive as long as the
    tensor's storage, and the block is freed with it).  The block is not
    torch's: it does not show in torch.cuda.memory_allocated() or the caching
    allocator's statistics."""

    _hip = None

    def __init__(self, shape, dtype, dev):
        if _HipBlock._hip is None:
            _HipBlock._hip = ctypes.CDLL("libamdhip64.so")
        hip = _HipBlock._hip
        self.ptr = ctypes.c_void_p()
        nbytes = int(np.prod(shape)) * torch.tensor([], dtype=dtype).element_size()
        with torch.cuda.device(dev):
            rc = hip.hipExtMallocWithFlags(ctypes.byref(self.ptr), ctypes.c_size_t(nbytes),
                                           ctypes.c_uint(0x4))       # hipDeviceMallocContiguous
        if rc != 0 or not self.ptr.value:
            self.ptr = None
            raise MemoryError(f"hipExtMallocWithFlags(contiguous, {nbytes}) failed: {rc}")
        typestr = {torch.float32: "<f4", torch.float64: "<f8"}[dtype]
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr,
                                         "data": (self.ptr.value, False), "version": 2,
                                         "strides": None}

    def __del__(self):
        # at interpreter shutdown the HIP runtime (or ctypes) may already be
        # gone: the process exit releases the memory then
        if getattr(self, "ptr", None) is None or _HipBlock._hip is None or sys.is_finalizing():
            return
        try:
            _HipBlock._hip.hipFree(self.ptr)
        except Exception:            # noqa: BLE001 -- never raise from a finaliser
            pass
        self.ptr = None


def _contiguous_empty(shape, dtype, dev) -> Optional[torch.Tensor]:
    """A device tensor in physically contiguous memory, or None."""
    if dtype not in (torch.float32, torch.float64):
        return None
    try:
        blk = _HipBlock(shape, dtype, dev)
        t = torch.as_tensor(blk, device=dev)
    except (OSError, MemoryError, RuntimeError, TypeError, KeyError):
        return None
    if t.data_ptr() != blk.ptr.value:            # torch copied instead of wrapping
        return None
    t._mf_block = blk                            # torch's storage deleter holds it too
    return t


# ------------------------------------------------------- host-side CSRs
def exclusion_csr(n_query: int, ex_ptr, ex_items, sort: bool):
    """The exclusion CSR of ``n_query`` queries as the kernels take it: (int64
    offsets rebased to 0, int32 items ex_items[ex_ptr[0]:ex_ptr[-1]]), each
    query's list ascending when ``sort`` (mf_topk and mf_rank binary-search
    it), a one-element dummy for an empty item array (never a null pointer);
    (None, None) without exclusions."""
    if ex_ptr is None:
        return None, None
    ex_ptr = np.ascontiguousarray(ex_ptr, np.int64)
    if len(ex_ptr) != n_query + 1:
        raise ValueError("ex_ptr needs n_query + 1 offsets")
    ex_items = np.ascontiguousarray(ex_items, np.int32)[ex_ptr[0]:ex_ptr[-1]]
    if sort:
        seg = np.repeat(np.arange(n_query, dtype=np.int64), np.diff(ex_ptr))
        ex_items = ex_items[np.lexsort((ex_items, seg))]
    return ex_ptr - ex_ptr[0], ex_items if len(ex_items) else np.zeros(1, np.int32)


def target_csr(n_query: int, tgt_ptr, tgt_items):
    """The target CSR of ``n_query`` queries, checked: (int64 offsets rebased
    to 0, the int32 items they cover, their number)."""
    tgt_ptr = np.ascontiguousarray(tgt_ptr, np.int64)
    tgt_items = np.ascontiguousarray(tgt_items, np.int32)
    if len(tgt_ptr) != n_query + 1:
        raise ValueError("tgt_ptr needs n_query + 1 offsets")
    tgt_ptr = tgt_ptr - tgt_ptr[0]
    nt = int(tgt_ptr[-1])
    if np.any(np.diff(tgt_ptr) < 0) or nt > len(tgt_items):
        raise ValueError("tgt_ptr must be non-decreasing and end within tgt_items")
    return tgt_ptr, tgt_items[:nt], nt


# ---------------------------------------------------------------- model
class DeviceModel:
    """Factor-model parameters on one GPU, and the scoring entry points.

    ``kernel`` is ``"linear" | "sigmoid" | "rbf"`` (KernelMF) or ``"bias"``
    (BaselineModel: no factor matrices).  The parameters start unset:
    ``load_params`` uploads them.
    """

    def __init__(self, n_users: int, n_items: int, n_factors: int, kernel: str,
                 dtype="float64", device=None, gamma: float = 0.0,
                 min_rating: float = 0.0, max_rating: float = 5.0,
                 global_mean: float = 0.0):
        self.dev = resolve_device(device)
        _warm_device(self.dev)
        self.dtype = canonical_dtype(dtype)
        self.tdt, self.ndt, self.dcode = DTYPES[self.dtype]
        self.kernel = kernel
        self.bias_only = kernel == "bias"
        if not self.bias_only:
            if kernel not in _lib.KERNEL_CODES:
                raise ValueError(f"unknown kernel {kernel!r}")
            self.kcode = _lib.KERNEL_CODES[kernel]
            kmax = _lib.load().mf_max_factors()
            if not 0 <= n_factors <= kmax:
                raise ValueError(f"n_factors must be in [0, {kmax}], got {n_factors}")
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.k = int(n_factors)
        self.gamma = float(gamma)
        self.min_rating, self.max_rating = float(min_rating), float(max_rating)
        self.global_mean = float(global_mean)
        self.P = self.Q = self.bu = self.bi = None

    # ---------------------------------------------------------- plumbing
    @property
    def stream(self):
        return _VOID(torch.cuda.current_stream(self.dev).cuda_stream)

    def _dev(self, a, shape) -> torch.Tensor:
        if isinstance(a, torch.Tensor):
            t = a.to(device=self.dev, dtype=self.tdt)
        else:
            t = torch.from_numpy(np.ascontiguousarray(a, self.ndt)).to(self.dev)
        t = t.reshape(shape).contiguous()
        return t

    def _dev_rows(self, a, shape) -> torch.Tensor:
        """P in physically contiguous device memory (hipExtMallocWithFlags,
        hipDeviceMallocContiguous) from 16 MiB up.  Every sweep reads and
        writes the user rows at random; measured at C3 (tools/layout_probe.py,
        profiles/r03/layout_probe_contiguous_r03s31.json)
        the sweep takes 9.45 ms with P contiguous and 10.1 ms when P lands in
        memory the allocator assembled from smaller pieces (most likely the
        address-translation fragment size), which happened in every process
        but bench.py's.  Falls back to an ordinary allocation if the runtime
        refuses; MF_CONTIGUOUS_ROWS=0 turns it off."""
        t = self._dev(a, shape)
        nbytes = t.numel() * t.element_size()
        if (os.environ.get("MF_CONTIGUOUS_ROWS") == "0" or self.dev.type != "cuda"
                or nbytes < (16 << 20)):
            return t
        v = _contiguous_empty(shape, t.dtype, self.dev)
        if v is None:
            return t
        v.copy_(t)
        return v

    def load_params(self, P=None, Q=None, bu=None, bi=None) -> None:
        """Upload parameters (NumPy or torch); None keeps the current one."""
        if P is not None:
            self.P = self._dev_rows(P, (self.n_users, self.k))
        if Q is not None:
            self.Q = self._dev(Q, (self.n_items, self.k))
        if bu is not None:
            self.bu = self._dev(bu, (self.n_users,))
        if bi is not None:
            self.bi = self._dev(bi, (self.n_items,))

    def params_numpy(self):
        """(P, Q, b_u, b_i) as float64 host arrays (synchronises)."""
        out = []
        for t in (self.P, self.Q, self.bu, self.bi):
            out.append(None if t is None else t.cpu().numpy().astype(np.float64))
        return tuple(out)

    def _model_args(self) -> tuple:
        """The model as mf_topk, mf_rank and mf_hybrid_rerank take it
        (include/mf_hip.h: global mean, biases, factors, n_items, n_factors,
        kernel, dtype, gamma, rating bounds); mf_topk_mm takes the first nine."""
        return (self.global_mean, _tp(self.bu), _tp(self.bi), _tp(self.P), _tp(self.Q),
                self.n_items, self.k, self.kcode, self.dcode, self.gamma, self.min_rating,
                self.max_rating)

    # ----------------------------------------------------------- scoring
    def predict(self, u: np.ndarray, i: np.ndarray, bound: bool) -> np.ndarray:
        """Predictions for id pairs (-1 = unknown), float64 host array."""
        n = len(u)
        if n == 0:
            return np.empty(0, np.float64)
        ud = torch.from_numpy(np.ascontiguousarray(u, np.int32)).to(self.dev)
        idd = torch.from_numpy(np.ascontiguousarray(i, np.int32)).to(self.dev)
        out = torch.empty(n, dtype=self.tdt, device=self.dev)
        with torch.cuda.device(self.dev):
            if self.bias_only:
                _lib.call("mf_bias_predict", _tp(ud), _tp(idd), n, self.global_mean,
                          _tp(self.bu), _tp(self.bi), self.dcode, self.min_rating,
                          self.max_rating, int(bound), _tp(out), self.stream)
            else:
                _lib.call("mf_predict", _tp(ud), _tp(idd), n, self.global_mean,
                          _tp(self.bu), _tp(self.bi), _tp(self.P), _tp(self.Q), self.k,
                          self.kcode, self.dcode, self.gamma, self.min_rating,
                          self.max_rating, int(bound), _tp(out), self.stream)
        return out.cpu().numpy().astype(np.float64)

    # workspace of one top-k launch (fused path: the partial lists; two-stage
    # path, amount > 64: n_query * n_items * 8 B of keys); users beyond this
    # budget go in further launches
    topk_ws_budget = 1 << 30
    # recommend_batch through the MFMA candidate filter where supported
    # (mf_topk_mm; env MF_TOPK_MFMA=0 forces the exact kernels)
    topk_mfma = True

    def topk_prepare(self, users: np.ndarray, amount: int,
                     ex_ptr: Optional[np.ndarray] = None,
                     ex_items: Optional[np.ndarray] = None) -> dict:
        """Device-resident top-k batch: query ids, exclusion CSR (each user's
        list sorted, as the fused kernel binary-searches it), workspace and
        outputs, and the users per launch (``topk_ws_budget``)."""
        if self.bias_only:
            raise NotImplementedError("top-k is implemented for factor models")
        users = np.ascontiguousarray(users, np.int32)
        nq = len(users)
        q = {"nq": nq, "amount": int(amount)}
        if nq == 0 or amount == 0:
            return q
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)  # noqa: E731
        q["users"] = to(users)
        ex_ptr, ex_items = exclusion_csr(nq, ex_ptr, ex_items, sort=True)
        q["ex_ptr"] = None if ex_ptr is None else to(ex_ptr)
        q["ex_items"] = None if ex_ptr is None else to(ex_items)
        lib = _lib.load()
        q["mm"] = (self.topk_mfma and os.environ.get("MF_TOPK_MFMA") != "0" and
                   bool(lib.mf_topk_mm_supported(self.k, self.kcode, self.dcode, amount)))
        self._topk_workspace(q, q["mm"])
        q["items"] = torch.empty((nq, amount), dtype=torch.int32, device=self.dev)
        q["scores"] = torch.empty((nq, amount), dtype=self.tdt, device=self.dev)
        q["ovf"] = torch.zeros(1, dtype=torch.int32, device=self.dev)
        return q

    def _topk_workspace(self, q: dict, mm: bool) -> None:
        """Users per launch (grid limits, then halved until the workspace fits
        ``topk_ws_budget``) and the workspace, for the MFMA-filter path
        (mf_topk_mm) or the exact one (mf_topk)."""
        lib = _lib.load()
        nq, amount = q["nq"], q["amount"]
        need = ((lambda c: lib.mf_topk_mm_workspace_bytes(c, self.n_items)) if mm else
                (lambda c: lib.mf_topk_workspace_bytes(c, self.n_items, amount)))
        chunk = min(nq, 65535 if amount > 64 else 1 << 20)
        while chunk > 1 and need(chunk) > self.topk_ws_budget:
            chunk = (chunk + 1) // 2
        q["chunk"] = chunk
        q["ws"] = torch.empty(max(need(chunk), 8), dtype=torch.uint8, device=self.dev)

    def topk_launch(self, q: dict, exact: bool = False) -> None:
        """Enqueue the top-k of a prepared batch (results stay on the device):
        mf_topk_mm where supported (its overflow word in q["ovf"]), else, or
        with ``exact``, mf_topk."""
        nq, amount = q["nq"], q["amount"]
        if nq == 0 or amount == 0:
            return
        mm = q["mm"] and not exact
        if not mm and q.get("mm"):
            self._topk_workspace(q, False)        # the exact path's workspace
            q["mm"] = False
        chunk = q["chunk"]
        es_i, es_s = q["items"].element_size(), q["scores"].element_size()
        if mm:
            q["ovf"].zero_()
        model = self._model_args()
        with torch.cuda.device(self.dev):
            for q0 in range(0, nq, chunk):
                q1 = min(nq, q0 + chunk)
                # CSR offsets stay absolute: the chunk's ptr array starts at row q0
                dp = None if q["ex_ptr"] is None else _VOID(q["ex_ptr"].data_ptr() + 8 * q0)
                users = _VOID(q["users"].data_ptr() + 4 * q0)
                items = _VOID(q["items"].data_ptr() + es_i * amount * q0)
                scores = _VOID(q["scores"].data_ptr() + es_s * amount * q0)
                if mm:
                    _lib.call("mf_topk_mm", users, q1 - q0, *model[:9], dp, _tp(q["ex_items"]),
                              amount, _tp(q["ws"]), items, scores, _tp(q["ovf"]), self.stream)
                else:
                    _lib.call("mf_topk", users, q1 - q0, *model, dp, _tp(q["ex_items"]),
                              amount, _tp(q["ws"]), items, scores, self.stream)

    def topk_finish(self, q: dict) -> bool:
        """After topk_launch: if the MFMA filter overflowed, re-run the exact
        path (synchronises).  Returns whether it had to."""
        if not q.get("mm") or q["nq"] == 0 or q["amount"] == 0:
            return False
        if int(q["ovf"].item()) == 0:
            return False
        self.topk_launch(q, exact=True)
        return True

    def topk(self, users: np.ndarray, amount: int, ex_ptr: Optional[np.ndarray] = None,
             ex_items: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Best ``amount`` items per internal user id: (item ids, scores).

        ``ex_ptr`` / ``ex_items``: optional CSR exclusions (query q skips
        items ex_items[ex_ptr[q]:ex_ptr[q+1]])."""
        q = self.topk_prepare(users, amount, ex_ptr, ex_items)
        if q["nq"] == 0 or amount == 0:
            return (np.full((q["nq"], amount), -1, np.int32),
                    np.full((q["nq"], amount), np.nan, np.float64))
        self.topk_launch(q)
        self.topk_finish(q)
        return q["items"].cpu().numpy(), q["scores"].cpu().numpy().astype(np.float64)

    # workspace of one rank launch (16 B per target); users whose targets go
    # beyond this budget take further launches (one user's targets never split)
    rank_ws_budget = 1 << 30

    def rank(self, users: np.ndarray, tgt_ptr: np.ndarray, tgt_items: np.ndarray,
             ex_ptr: Optional[np.ndarray] = None,
             ex_items: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Exact rank of each target item among its user's candidates (mf_rank):
        (ranks int32[n_targets], n_candidates int32[n_query]).

        ``tgt_ptr`` / ``tgt_items``: CSR targets per internal user id in
        ``users`` (any order, repeats allowed).  ``ex_ptr`` / ``ex_items``:
        optional CSR exclusions as for ``topk``.  A target that is out of
        range or excluded for its user gets rank -1."""
        if self.bias_only:
            raise NotImplementedError("ranking is implemented for factor models")
        users = np.ascontiguousarray(users, np.int32)
        nq = len(users)
        tgt_ptr, tgt_items, nt = target_csr(nq, tgt_ptr, tgt_items)
        if nq == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)  # noqa: E731
        d_users = to(users)
        ex_ptr, ex_items = exclusion_csr(nq, ex_ptr, ex_items, sort=True)
        d_ex_ptr = None if ex_ptr is None else to(ex_ptr)
        d_ex_items = None if ex_ptr is None else to(ex_items)
        d_tgt_items = to(tgt_items if nt else np.zeros(1, np.int32))
        ranks = torch.empty(max(nt, 1), dtype=torch.int32, device=self.dev)
        cands = torch.empty(nq, dtype=torch.int32, device=self.dev)
        lib = _lib.load()
        # user chunks: the longest runs whose targets fit the workspace budget
        cap = max(1, self.rank_ws_budget // max(1, lib.mf_rank_workspace_bytes(1, 1, self.n_items)))
        bounds = [0]
        while bounds[-1] < nq:
            q0 = bounds[-1]
            q1 = int(np.searchsorted(tgt_ptr, tgt_ptr[q0] + cap, side="right")) - 1
            bounds.append(min(nq, max(q1, q0 + 1)))
        model = self._model_args()
        with torch.cuda.device(self.dev):
            for q0, q1 in zip(bounds[:-1], bounds[1:]):
                b0, b1 = int(tgt_ptr[q0]), int(tgt_ptr[q1])
                d_ptr = to(tgt_ptr[q0:q1 + 1] - b0)      # chunk-relative offsets
                ws = torch.empty(max(lib.mf_rank_workspace_bytes(q1 - q0, b1 - b0, self.n_items),
                                     16), dtype=torch.uint8, device=self.dev)
                # exclusion offsets stay absolute: the chunk's ptr array starts at row q0
                dp = None if d_ex_ptr is None else _VOID(d_ex_ptr.data_ptr() + 8 * q0)
                _lib.call("mf_rank", _VOID(d_users.data_ptr() + 4 * q0), q1 - q0, *model, dp,
                          _tp(d_ex_items), _tp(d_ptr), _VOID(d_tgt_items.data_ptr() + 4 * b0),
                          _tp(ws), _VOID(ranks.data_ptr() + 4 * b0),
                          _VOID(cands.data_ptr() + 4 * q0), self.stream)
        return ranks[:nt].cpu().numpy(), cands.cpu().numpy()
