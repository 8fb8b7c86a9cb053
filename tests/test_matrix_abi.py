"""The distance matrix API is part of the C-ABI and of the Python package: the library loads on a CPU-only box and exports qmx_sample_points and
qmx_search_matrix, the addition left the ABI version alone, and the argument checks that need no device answer as the header says.  CPU only."""
import ctypes as C


def test_library_exports_the_matrix_entry_points():
    from qdrant_amd import _ffi
    lib = _ffi.lib()
    for name in ("qmx_sample_points", "qmx_search_matrix"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name), name
    assert lib.qmx_abi_version() == 8      # purely additive


def test_python_surface():
    import qdrant_amd as qa
    from qdrant_amd import matrix
    for name in ("sample_points", "search_matrix", "search_matrix_pairs", "search_matrix_offsets", "SearchMatrix"):
        assert callable(getattr(qa, name)), name
    # the reference's defaults (CollectionSearchMatrixRequest::DEFAULT_SAMPLE / DEFAULT_LIMIT_PER_SAMPLE)
    assert matrix.DEFAULT_SAMPLE == 10 and matrix.DEFAULT_LIMIT_PER_SAMPLE == 3
    assert qa.search_matrix_pairs.__defaults__[:2] == (10, 3) and qa.search_matrix_offsets.__defaults__[:2] == (10, 3)


def test_null_arguments_are_refused_before_any_device_work():
    from qdrant_amd import _ffi as F
    lib = F.lib()
    count = C.c_uint32(7)
    assert lib.qmx_sample_points(None, None, 0, 4, 0, None, C.cast(C.byref(count), C.c_void_p)) == F.ERR_BAD_ARG
    assert lib.qmx_search_matrix(None, None, 3, 3, None, None, None, None) == F.ERR_BAD_ARG
