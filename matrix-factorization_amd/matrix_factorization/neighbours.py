"""Device-side state of the neighbourhood models (ItemItemCF / UserUserCF).

One engine serves both classes: the ENTITIES are the items (ItemItemCF) or the
users (UserUserCF), the OTHERS are the other side.  The fitted triples are
sorted into both CSR orientations on the device (entity-major with each list
ascending in the other's id, other-major with each list ascending in the
entity's id: the order mf_cf_similarity's bitwise symmetry rests on), the
statistics and the similarity are computed once (mf_cf_stats,
mf_cf_similarity), and predict() scores pairs in chunks (mf_cf_predict).
Ratings are float32 on the device; means, norms and predictions are FP64.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .engine import _VOID, _tp, resolve_device

DEFAULT_MAX_SIMILARITY_BYTES = 16 << 30      # policy, not a measurement
PREDICT_CHUNK = 1 << 20                      # pairs per mf_cf_predict launch (<= 2^25)


def similarity_bytes(n_entities: int) -> int:
    return 4 * int(n_entities) * int(n_entities)


def check_similarity_bytes(n_entities: int, max_bytes: int, what: str = "entities") -> None:
    """Refuse, before anything is allocated, a similarity matrix larger than
    ``max_bytes``."""
    need = similarity_bytes(n_entities)
    if need > max_bytes:
        raise ValueError(
            f"the {n_entities} x {n_entities} float32 similarity matrix of {n_entities} {what} "
            f"needs {need} bytes ({need / 2**30:.2f} GiB), more than max_similarity_bytes="
            f"{max_bytes}")


class NeighbourEngine:
    """CSR lists, statistics and similarity of one fitted neighbourhood model.

    ent, oth, r: the training triples (internal ids, one rating per pair).
    Attributes: mean, norm (float64 device tensors, n_entities), S (float32
    device tensor, n_entities x n_entities)."""

    def __init__(self, ent: np.ndarray, oth: np.ndarray, r: np.ndarray, n_entities: int,
                 n_others: int, device=None,
                 max_similarity_bytes: int = DEFAULT_MAX_SIMILARITY_BYTES,
                 pass_cols: int = 0, what: str = "entities"):
        check_similarity_bytes(n_entities, max_similarity_bytes, what)
        ent = np.asarray(ent, dtype=np.int64)
        oth = np.asarray(oth, dtype=np.int64)
        if len(ent) and (ent.min() < 0 or ent.max() >= n_entities
                         or oth.min() < 0 or oth.max() >= n_others):
            raise ValueError("rating ids outside [0, n_entities) x [0, n_others)")
        self.dev = resolve_device(device)
        self.n_entities, self.n_others = int(n_entities), int(n_others)
        with torch.cuda.device(self.dev):
            d_ent = torch.from_numpy(ent).to(self.dev)
            d_oth = torch.from_numpy(oth).to(self.dev)
            d_r = torch.from_numpy(np.asarray(r, dtype=np.float32)).to(self.dev)
            self.entity_csr = self._csr(d_ent, d_oth, d_r, self.n_entities, self.n_others)
            self.other_csr = self._csr(d_oth, d_ent, d_r, self.n_others, self.n_entities)
            self.mean = torch.empty(self.n_entities, dtype=torch.float64, device=self.dev)
            self.norm = torch.empty(self.n_entities, dtype=torch.float64, device=self.dev)
            self.S = torch.empty((self.n_entities, self.n_entities), dtype=torch.float32,
                                 device=self.dev)
            eptr, eoth, er = self.entity_csr
            optr, oent, orr = self.other_csr
            _lib.call("mf_cf_stats", _tp(eptr), _tp(er), self.n_entities, self.n_others,
                      _lib.MF_F32, _tp(self.mean), _tp(self.norm), self.stream)
            _lib.call("mf_cf_similarity", _tp(eptr), _tp(eoth), _tp(er), _tp(optr), _tp(oent),
                      _tp(orr), self.n_entities, self.n_others, _lib.MF_F32, _tp(self.mean),
                      _tp(self.norm), int(pass_cols), _tp(self.S), self.stream)

    @property
    def stream(self):
        return _VOID(torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def _csr(major, minor, r, n_major, n_minor):
        """(int64 offsets, int32 minor ids, float32 ratings) sorted by (major,
        minor), built on the device."""
        order = torch.argsort(major * max(n_minor, 1) + minor)
        ptr = torch.zeros(n_major + 1, dtype=torch.int64, device=major.device)
        if major.numel():
            torch.cumsum(torch.bincount(major, minlength=n_major), 0, out=ptr[1:])
        return ptr, minor[order].to(torch.int32).contiguous(), r[order].contiguous()

    def synchronize(self) -> None:
        torch.cuda.current_stream(self.dev).synchronize()

    def predict(self, ent: np.ndarray, oth: np.ndarray, n_neighbors: int, global_mean: float,
                min_rating: float, max_rating: float, bound: bool) -> np.ndarray:
        """FP64 predictions for the pairs (ent[p], oth[p]); -1 = unknown id."""
        n = len(ent)
        out = torch.empty(n, dtype=torch.float64, device=self.dev)
        optr, oent, orr = self.other_csr
        with torch.cuda.device(self.dev):
            d_e = torch.from_numpy(np.ascontiguousarray(ent, dtype=np.int32)).to(self.dev)
            d_o = torch.from_numpy(np.ascontiguousarray(oth, dtype=np.int32)).to(self.dev)
            for c0 in range(0, n, PREDICT_CHUNK):
                m = min(PREDICT_CHUNK, n - c0)
                _lib.call("mf_cf_predict", _VOID(d_e.data_ptr() + 4 * c0),
                          _VOID(d_o.data_ptr() + 4 * c0), m, _tp(optr), _tp(oent), _tp(orr),
                          _tp(self.S), _tp(self.mean), self.n_entities, self.n_others,
                          _lib.MF_F32, int(n_neighbors), float(global_mean), float(min_rating),
                          float(max_rating), int(bool(bound)), _VOID(out.data_ptr() + 8 * c0),
                          self.stream)
        return out.cpu().numpy()
