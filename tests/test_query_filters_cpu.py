"""qmx_query_set_filters without a device: the symbol is carried by the header, the binding and INTEGRATION.md with one signature; RawScorer.set_filters
packs its masks into the documented word layout (scorer.pack_filters, split from the call for this test); the ABI version did not move."""
import os
import re

import numpy as np
import pytest

from test_integration_doc import _header_decls, _rust_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qmx_query_set_filters"


def test_header_binding_and_integration_doc_carry_the_symbol():
    import ctypes as C
    from qdrant_amd import _ffi as F
    header = open(os.path.join(ROOT, "include", "qdrant_amd.h")).read()
    assert re.search(r"#define\s+QMX_FILTER_NONE\s+0xFFFFFFFFu\b", header)
    want = ["*mut QmxQuery", "*const u64", "u64", "u32", "*const u32"]
    assert _header_decls()[NAME] == ("i32", want)
    assert [(ret, params) for name, ret, params in _rust_decls() if name == NAME] == [("i32", want)]
    res, args = F.SIGNATURES[NAME]
    assert res is C.c_int32 and args == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    assert F.FILTER_NONE == 0xFFFFFFFF
    assert hasattr(F.lib(), NAME)


def test_set_filters_packs_the_documented_word_layout():
    from qdrant_amd.scorer import RawScorer, pack_filters
    assert hasattr(RawScorer, "set_filters")
    rng = np.random.default_rng(3)
    n_filters, n = 3, 200                                  # 200 bits: four words, the last one partly used
    masks = rng.random((n_filters, n)) < 0.4
    masks[0] = False
    masks[1, [0, 63, 64, 127, 128, 199]] = True
    words, n_bits, nf, fof = pack_filters(masks, [2, None, 0, -1, 1], 5)
    assert (n_bits, nf) == (n, n_filters)
    assert words.dtype == np.uint64 and words.shape == (n_filters, 4) and words.flags["C_CONTIGUOUS"]
    assert fof.dtype == np.uint32 and fof.tolist() == [2, 0xFFFFFFFF, 0, 0xFFFFFFFF, 1]
    for f in range(n_filters):                             # BitSlice<u64, Lsb0>: bit i = bit (i % 64) of word (i / 64); nothing set past n
        for i in range(256):
            bit = (int(words[f, i >> 6]) >> (i & 63)) & 1
            assert bit == (int(masks[f, i]) if i < n else 0), (f, i)
    # a multiple of 64 bits: no padding word
    words, n_bits, nf, fof = pack_filters(np.ones((1, 128), dtype=bool), [0], 1)
    assert words.shape == (1, 2) and words.tolist() == [[2 ** 64 - 1, 2 ** 64 - 1]]
    # one entry per query, at least one mask
    with pytest.raises(ValueError):
        pack_filters(masks, [0, 1], 5)
    with pytest.raises(ValueError):
        pack_filters(np.zeros((0, n), dtype=bool), [None] * 5, 5)
    with pytest.raises(ValueError):
        pack_filters(np.zeros(n, dtype=bool), [0] * 5, 5)


def test_the_abi_version_is_still_8():
    from qdrant_amd import _ffi as F
    assert F.lib().qmx_abi_version() == 8
