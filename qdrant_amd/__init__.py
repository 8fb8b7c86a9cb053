"""qdrant_amd — MI355X-native (gfx950, HIP) implementation of Qdrant's batched vector-scoring path.

Layout: `csrc/` (HIP kernels + the C-ABI of include/qdrant_amd.h), `_ffi.py` (ctypes binding),
`scorer.py` (host-side mirror of the reference's RawScorer / BatchFilteredSearcher interface).
"""
from ._ffi import (COSINE, DOT, DTYPE_BQ, DTYPE_F16, DTYPE_F32, DTYPE_PQ, DTYPE_SQ_U8, DTYPE_U8, EUCLID, FILTER_NONE, MANHATTAN,  # noqa: F401
                   QmxError, get_option, lib, set_option)
from .scorer import (BatchFilteredSearcher, Distance, EncodedVectorsPQ, EncodedVectorsU8, ProductQuantizer, RawScorer, ScalarQuantizer,  # noqa: F401
                     ScoredPointOffset, VectorStorage, VectorStorageDatatype, device_count, new_raw_scorer,
                     new_raw_scorer_internal, pq_train, search_quantized, CustomQuery, CustomRawScorer, BinaryQuantizer, EncodedVectorsBin, load_quantizer, MultiDenseVectorStorage, QuantizedMultivectorStorage, TurboQuantizer, EncodedVectorsTQ, vector_stats,
                     SparseVectorStorage, pack_filters)
from .groups import GroupKeys, search_groups  # noqa: F401
from .matrix import SearchMatrix, sample_points, search_matrix, search_matrix_offsets, search_matrix_pairs  # noqa: F401
from .hnsw import GraphLayers, decode_links_file, select_payload_blocks  # noqa: F401
from .query import Dbsf, Mmr, Rrf, dbsf, hybrid_search, mmr, rrf, sparse_mmr  # noqa: F401
from .query import (CompiledFormula, Formula, FormulaError, PayloadColumns, abs_, condition, const, datetime, decay_params_to_lambda,  # noqa: F401
                    div, exp, exp_decay, formula_eval, formula_rescore, gauss_decay, geo_distance, lin_decay, ln, log10, mult, neg, payload,
                    pow_, score, sqrt, sum_)
