"""CPU tests of the ctypes prototypes: _capi.SIGNATURES is read from include/dynaalign.h (header_prototypes), so what is checked here is
the reader -- names, every type kind against rows written out by hand, and that header text it does not understand is refused with the
function's name instead of getting a default type."""
import ctypes as C

import pytest

from dynaalign_amd import _capi

_vp, _i64, _i32, _u32, _sz, _f64, _str = C.c_void_p, C.c_int64, C.c_int, C.c_uint32, C.c_size_t, C.c_double, C.c_char_p

# full rows of the hand-written table this reader replaced, one or more per type kind
ROWS = {
    "da_last_error": (_str, []),
    "da_status_message": (_str, [_i32]),
    "da_edges_free": (None, [_vp]),
    "da_config_reload": (None, []),
    "da_random_seed": (_u32, []),
    "da_debug_comm_cache_state": (_i32, [_i32, _vp]),
    "da_dev_lsh_workspace_bytes": (_sz, [_i64, _i32]),
    "da_sig_ld": (_i64, [_i32]),
    "da_similarity_nw": (_i32, [_vp, _vp, _i64, _str, _i32, _i32, _vp]),
    "da_dev_threshold_ranks_count": (_i32, [_vp, _i64, _i64, _i64, _u32, _i64, _i32, _i64, _i64, _vp, _vp, _sz, _vp]),
    "da_dev_louvain_csr": (_i32, [_i64, _vp, _vp, _vp, _vp, _vp, _i32, _f64, _u32, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "da_dev_lsh_nw_edges": (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _f64, _i64, _vp, _vp, _i32, _i32, _i32, _f64, _vp, _sz, _vp, _vp,
                                   _vp, _vp, _i64, _vp, _vp]),
    "da_dev_lsh_cross_nw_edges": (_i32, [_vp, _sz, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _f64, _i64, _vp, _vp, _vp, _vp, _i32,
                                         _i32, _i32, _f64, _vp, _sz, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
}


def test_parsed_names_are_the_declared_names():
    parsed = _capi.header_prototypes()
    assert sorted(parsed) == _capi.header_symbols()
    assert parsed == _capi.SIGNATURES and isinstance(_capi.SIGNATURES, dict)
    for name, (res, args) in parsed.items():
        assert isinstance(args, list), name


@pytest.mark.parametrize("name", sorted(ROWS))
def test_row_equals_the_hand_written_row(name):
    assert _capi.SIGNATURES[name] == ROWS[name]
    assert len(_capi.SIGNATURES["da_dev_lsh_cross_nw_edges"][1]) == 30


def test_every_prototype_is_applied_to_the_loaded_library(built):
    lib = _capi.load()
    assert len(_capi.SIGNATURES) >= 171
    for name, (res, args) in _capi.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_type_spellings_the_reader_accepts():
    got = _capi.header_prototypes(text="""
        /* da_in_a_comment(float x); */
        #define DA_MACRO(x) da_not_a_function(x)
        extern DA_API const char *da_a(void);   // da_after_slashes(float);
        void da_b(int, const struct da_opts *opts, const char *const *names, int32_t v, uint32_t u, size_t s, double d, int64_t
                  wrapped);
        void *da_c();
    """)
    assert got == {"da_a": (_str, []), "da_b": (None, [_i32, _vp, _vp, _i32, _u32, _sz, _f64, _i64]), "da_c": (_vp, [])}


@pytest.mark.parametrize("text, name", [
    ("int da_x(int n);\nint da_unknown_scalar(float x, int n);", "da_unknown_scalar"),
    ("int da_unknown_scalar2(uint16_t x);", "da_unknown_scalar2"),
    ("unsigned da_unknown_return(void);", "da_unknown_return"),
    ("int da_void_value(void x);", "da_void_value"),
    ("int da_callback(void (*cb)(int), int n);", "da_callback"),
    ("int da_array(int n, int a[4]);", "da_array"),
    ("int da_split(int n\n#ifdef X\n, int m\n#endif\n;\nint da_y(void);", "da_split"),
    ("int da_ok(void);\nint da_no_semicolon(int n)\nint da_z(void);", "da_no_semicolon"),
])
def test_text_the_reader_does_not_understand_is_refused_by_name(text, name):
    with pytest.raises(ValueError, match=r"^%s: " % name):
        _capi.header_prototypes(text=text)
