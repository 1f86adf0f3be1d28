"""CPU: the ctypes binding is read from include/mgf.h (morphganformer_amd/_lib.py: parse_header).  The parser's rules on a literal header,
hand-written expectations for exports of the real header that between them use every C type it knows, the constants against their values
written out here, and the loaded library."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

I, I32, I64, U64, F32, F64, P = C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_void_p

MINI = """
/* int mgf_in_a_block_comment(int a);
 * int mgf_in_its_second_line(void); */
#ifndef MINI_H_
#define MINI_H_
#define MGF_MAX_THINGS 7
typedef void* mgf_stream_t; // int mgf_after_a_typedef(int a);
enum { MGF_ONE = 1, MGF_MINUS = -3 };
enum { MGF_A = 0,
       /* a comment between enumerators */
       MGF_B = 12 };
typedef struct mgf_rec {
    const float* p;   /* fields are no prototypes */
    int32_t n;
} mgf_rec;
const char* mgf_text(void);
int64_t mgf_count();
void mgf_nothing(int flag);
int32_t mgf_scalars(int a, int32_t b, int64_t c, uint64_t d, float e, double f, mgf_stream_t stream);
int mgf_pointers(void* y, const void* x, const float* const* maps, float** outs, const mgf_rec* rec, mgf_rec *jobs_dev,
                 const int32_t* sides_host,
                 const
                 double *  counts_host,  int32_t
                 n,
                 mgf_stream_t stream);
int mgf_unnamed(int32_t, const float*, mgf_stream_t);
// int mgf_in_a_line_comment(int a);
#endif
"""


def test_parser_rules_on_a_literal_header():
    from morphganformer_amd import _lib
    sigs, consts = _lib.parse_header(MINI)
    assert sigs == {
        "mgf_text": (C.c_char_p, []),
        "mgf_count": (I64, []),
        "mgf_nothing": (None, [I]),
        "mgf_scalars": (I32, [I, I32, I64, U64, F32, F64, P]),
        "mgf_pointers": (I, [P, P, P, P, P, P, P, P, I32, P]),
        "mgf_unnamed": (I, [I32, P, P]),
    }
    assert consts == {"MGF_MAX_THINGS": 7, "MGF_ONE": 1, "MGF_MINUS": -3, "MGF_A": 0, "MGF_B": 12}


@pytest.mark.parametrize("decl, names", [
    ("int mgf_bad(size_t n);", ["size_t", "mgf_bad"]),                                   # a scalar outside the rules: never `int` by default
    ("int mgf_bad(uint32_t flags, mgf_stream_t stream);", ["uint32_t", "mgf_bad"]),
    ("int mgf_bad(unsigned int n);", ["unsigned", "mgf_bad"]),
    ("int mgf_bad(int32_t sides[4]);", ["sides[4]", "mgf_bad"]),
    ("uint32_t mgf_bad(void);", ["uint32_t", "mgf_bad"]),
    ("float* mgf_bad(void);", ["float *", "mgf_bad"]),                                   # the one pointer result is `const char*`
    ("int mgf_bad(void (*callback)(int), mgf_stream_t stream);", ["mgf_bad"]),           # a function-pointer parameter
    ("#define MGF_DECLARE int mgf_bad(int32_t n);", ["mgf_bad"]),                        # a declaration inside a macro
    ("MGF_API(int) mgf_bad(int32_t n);", ["mgf_bad"]),
    ("enum { MGF_FIRST, MGF_SECOND };", ["MGF_FIRST"]),                                  # an implicit value
    ("enum { MGF_FLAG = 1 << 2 };", ["MGF_FLAG"]),
])
def test_parser_refuses_what_it_does_not_understand(decl, names):
    from morphganformer_amd import _lib
    good = "int mgf_good(int32_t n, mgf_stream_t stream);\n"
    assert "mgf_good" in _lib.parse_header(good)[0]
    with pytest.raises(_lib.MgfError) as e:
        _lib.parse_header(good + decl + "\n" + good.replace("good", "good2"))
    for name in names:
        assert name in str(e.value), (name, str(e.value))


def test_real_header_against_hand_written_signatures():
    """About a dozen exports that between them use every type of the rule set, written out independently of the parser."""
    from morphganformer_amd import _lib
    want = {
        "mgf_last_error": (C.c_char_p, []),
        "mgf_reduce_scratch_floats": (I64, []),
        "mgf_bwd_chunks": (I32, [I64]),
        "mgf_randn_f32": (I, [P, I64, U64, P, P]),
        "mgf_wing_loss_f64": (I, [P, P, P, I32, I64, F64, F64, P, I32, P]),
        "mgf_conv_taps_f32": (I, [P] * 8),                                                # ..., const mgf_conv_desc*, const mgf_epilogue*, stream
        "mgf_lpips_upsample_sum_f32": (I, [P, P, P, I32, I32, I32, I32, P]),              # const float* const* maps, const int32_t* sides
        "mgf_lpips_finish_taps_f32": (I, [P, P, I64, I32, P, P, I32, I32, P]),            # two host arrays
        "mgf_conv_profile_end": (I, [P, I32]),
        "mgf_upfirdn2d": (I, [P, P, P, I] + [I32] * 4 + [I64] * 4 + [I32] * 2 + [I64] * 4 + [I32] * 11 + [F32, P, P]),
        "mgf_mdf_finish_f32": (I, [P, P, I32, I64, P, I32, F32, I32, P]),
        "mgf_select_best": (I, [P] * 5 + [I64, P, P, P, F64, F32, P, P, I32, I32, P, P, I32, P, P, P]),
    }
    assert len(want["mgf_upfirdn2d"][1]) == 32
    for name, sig in want.items():
        assert _lib._SIGS[name] == sig, name
    used = {t for res, args in want.values() for t in [res] + args}
    assert used == {C.c_char_p, I, I32, I64, U64, F32, F64, P}
    assert _lib.EXPORTED_SYMBOLS == sorted(_lib._SIGS) and len(_lib.EXPORTED_SYMBOLS) >= 157


def test_constants_equal_the_values_written_out_here():
    from morphganformer_amd import _lib
    from morphganformer_amd.embedder import ArcFaceEmbedder
    assert (_lib.MGF_OK, _lib.MGF_EINVAL, _lib.MGF_EUNSUPPORTED, _lib.MGF_ELAUNCH, _lib.MGF_ETOOBIG) == (0, -1, -2, -3, -4)
    assert (_lib.MGF_F32, _lib.MGF_F64, _lib.MGF_F16) == (0, 1, 2)
    assert _lib.ACT_IDS == {"linear": 1, "relu": 2, "lrelu": 3, "tanh": 4, "sigmoid": 5, "elu": 6, "selu": 7, "softplus": 8, "swish": 9,
                            "relu_post": 10}
    assert _lib.MGF_ACT_LRELU == 3 and _lib.MGF_ACT_RELU_POST == 10
    assert (_lib.MGF_FILTER_SEPARABLE, _lib.MGF_FILTER_LARGE) == (2, 4)
    assert (_lib.MGF_CROP_AREA, _lib.MGF_CROP_BILINEAR) == (0, 1)
    assert ArcFaceEmbedder.CROP_FILTERS == {"area": 0, "bilinear": 1}
    assert _lib.MAX_TAPS == _lib.MGF_MAX_TAPS == 9
    assert all(type(v) is int for v in _lib.CONSTANTS.values()) and len(_lib.CONSTANTS) == 23


def test_library_loads_with_every_symbol_bound():
    from morphganformer_amd import _lib, build
    build.build()
    handle = _lib.lib()
    for name in _lib.EXPORTED_SYMBOLS:
        fn = getattr(handle, name)
        res, args = _lib._SIGS[name]
        assert fn.argtypes is not None and list(fn.argtypes) == args and fn.restype is res, name
    assert handle.mgf_version() >= 100 and isinstance(handle.mgf_last_error(), bytes)
    assert handle.mgf_bwd_chunks((1 << 32) + 1) > handle.mgf_bwd_chunks(1) == 1           # an int64_t argument arrives whole
