"""A numpy restatement of the reference's f16 / u8 index weights and of its IDF modifier (test infrastructure, CPU only).

* Weights (lib/sparse/src/common/types.rs; built per posting list in compressed_posting_list.rs:361-407): `half::f16::from_f32` (round to nearest
  even, exact widening back) or `QuantizedU8` with (min, diff256 = (max - min) / 255) per posting list:
  encode = ((v - min) / diff256).round().clamp(0, 255) as u8 - f32 division, round half AWAY from zero, NaN (0 / 0 of an all-equal list) -> 0;
  decode = min + f32(code) * diff256, the multiply and the add rounded separately.
* SearchContext::search / plain_search (search_context.rs:92-187) read the index: `WeightsRestatement` is sparse_reference.Restatement with the
  posting weights replaced by the decoded ones.  The raw scorer and the custom queries read the f32 vector storage: an f32 Restatement.
* IDF (segment/src/data_types/query_context.rs:275-299, sparse_vector_index/read_view/idf.rs): fancy_idf in f32 with `f32::ln` = glibc logf,
  called through ctypes (numpy's float32 log rounds differently); global and corpus statistics; remap_idf_weights over ORIGINAL indices.
"""
import ctypes
import ctypes.util

import numpy as np

import sparse_reference as SR

F32, F16, U8 = "f32", "f16", "u8"

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def round_half_away(x):
    """f32::round of a float32 array (half away from zero; np.round is half-to-even), NaN kept."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)      # |x| + 0.5 is exact in float64 for every float32 that is not an integer already
    return (np.sign(x64) * np.floor(np.abs(x64) + 0.5)).astype(np.float32)


def u8_params(weights):
    """QuantizedU8::quantization_params_for: (min, diff256) in float32."""
    w = np.asarray(weights, dtype=np.float32)
    if len(w) == 0:
        return np.float32(0.0), np.float32(0.0)
    mn, mx = w.min(), w.max()
    return np.float32(mn), np.float32(np.float32(mx - mn) / np.float32(255.0))


def u8_encode(weights, mn, d256):
    w = np.asarray(weights, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = (w - np.float32(mn)) / np.float32(d256)
    r = round_half_away(q)
    r = np.where(np.isnan(r), np.float32(0.0), np.clip(r, np.float32(0.0), np.float32(255.0)))      # clamp keeps NaN, `as u8` makes it 0
    return r.astype(np.uint8)


def u8_decode(codes, mn, d256):
    prod = np.asarray(codes).astype(np.float32) * np.float32(d256)
    return (np.float32(mn) + prod).astype(np.float32)


def f16_decode(weights):
    with np.errstate(over="ignore"):
        return np.asarray(weights, dtype=np.float32).astype(np.float16).astype(np.float32)


class WeightsRestatement(SR.Restatement):
    """Restatement whose index holds `weights` = "f32" / "f16" / "u8": `_post_w` are the decoded weights, posting list by posting list."""

    def __init__(self, rows, dim_map=None, weights=F32):
        super().__init__(rows, dim_map=dim_map)
        self.weights = weights
        self.stored_w = self._post_w.copy()          # the f32 weights, posting order
        if weights == F16:
            self._post_w = f16_decode(self._post_w)
        elif weights == U8:
            out = np.empty_like(self._post_w)
            self.params = []
            for k in range(len(self._dims)):
                a, b = self._starts[k], self._starts[k + 1]
                mn, d = u8_params(self.stored_w[a:b])
                self.params.append((mn, d))
                out[a:b] = u8_decode(u8_encode(self.stored_w[a:b], mn, d), mn, d)
            self._post_w = out
        else:
            assert weights == F32, weights

    # ---- IDF statistics (fill_idf_statistics) ----
    def _remapped(self, dim):
        if self.dim_map is None:
            return int(dim)
        return self.dim_map.get(int(dim))

    def global_statistics(self, dims):
        """df(d) = the whole posting length (deleted points included), n = the non-empty vectors indexed."""
        df = np.zeros(len(dims), dtype=np.uint64)
        for i, d in enumerate(dims):
            r = self._remapped(d)
            if r is not None:
                df[i] = len(self.postings(r)[0])
        return df, int(len(np.unique(self._post_rows)))

    def corpus_members(self, mask, point_deleted=None, vec_deleted=None):
        """The corpus points that are neither point- nor vector-deleted (a bool array over the rows; empty vectors count)."""
        member = np.zeros(self.n, dtype=bool)
        m = np.asarray(mask, dtype=bool)[:self.n]
        member[:len(m)] = m
        for flags in (point_deleted, vec_deleted):
            if flags is not None:
                f = np.asarray(flags, dtype=bool)[:self.n]
                member[:len(f)] &= ~f
        return member

    def corpus_statistics_mask(self, dims, member):
        """CorpusPoints::Mask: walk every posting list against the mask."""
        df = np.zeros(len(dims), dtype=np.uint64)
        for i, d in enumerate(dims):
            r = self._remapped(d)
            if r is not None:
                df[i] = int(np.count_nonzero(member[self.postings(r)[0]]))
        return df, int(np.count_nonzero(member))

    def corpus_statistics_ids(self, dims, member):
        """CorpusPoints::SortedIds: skip_to every corpus id in every posting list."""
        ids = np.flatnonzero(member)
        df = np.zeros(len(dims), dtype=np.uint64)
        for i, d in enumerate(dims):
            r = self._remapped(d)
            if r is None:
                continue
            rows = self.postings(r)[0]
            if len(rows) == 0:
                continue
            probe = ids[ids <= rows[-1]]
            at = np.searchsorted(rows, probe)
            df[i] = int(np.count_nonzero(rows[np.minimum(at, len(rows) - 1)] == probe))
        return df, len(ids)


def fancy_idf(n, df):
    """VectorQueryContext::fancy_idf: ((n - df + 0.5) / (df + 0.5) + 1).ln() in f32, n and df converted from integers."""
    n, df = np.float32(int(n)), np.float32(int(df))
    half, one = np.float32(0.5), np.float32(1.0)
    x = np.float32(np.float32(np.float32(np.float32(n - df) + half) / np.float32(df + half)) + one)
    return np.float32(_libm.logf(float(x)))


def remap_idf_weights(indices, values, dims, df, n_docs):
    """weight *= fancy_idf(n, df[original index]); df = 0 for an index without a statistic."""
    stat = {int(d): int(c) for d, c in zip(dims, df)}
    out = np.asarray(values, dtype=np.float32).copy()
    for k, ix in enumerate(indices):
        out[k] = np.float32(out[k] * fancy_idf(n_docs, stat.get(int(ix), 0)))
    return out


def merge_statistics(a, b):
    """Statistics of two segments over the same `dims`: df and n are added."""
    return a[0] + b[0], a[1] + b[1]
