"""ctypes binding of the C ABI in include/mgf.h (libmgf_hip.so, built in-tree by morphganformer_amd/build.py).

There is NO CPU fallback: if the shared library is missing, `lib()` raises, and every op checks that its tensors
live on a HIP device.  (The reference silently falls back to slow torch ops when its plugin build fails,
torch_utils/ops/bias_act.py:39-43; a drop-in for the GPU hot path must not.)

The header is the one statement of the ABI: the signature of every entry point and every MGF_* constant are read from it at import
(`parse_header`), so the compiler checks the definitions in csrc/ and this module against the same text.  Only the struct classes
below are written by hand (tests/test_host_and_abi.py compares their layouts with a C compiler's).
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGF_LIB_PATH") or os.path.join(HERE, "libmgf_hip.so")     # env override: kernel experiments only
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "mgf.h")                # (csrc/mgf_common.h includes it by the same relative path)

i32, i64, f32, f64, vp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p


class MgfError(RuntimeError):
    pass


# One rule per C type of the header.  Every pointer parameter is c_void_p -- struct pointers too: `const mgf_style_job*` is a host
# struct (byref) in one entry and a device address (int) in another, and c_void_p takes None, int, byref(...) and ctypes arrays alike.
# A type outside the rules is refused, never bound as int by default.
_SCALARS = {"int": C.c_int, "int32_t": i32, "int64_t": i64, "uint64_t": C.c_uint64, "float": f32, "double": f64, "mgf_stream_t": vp}
_PROTOTYPE = re.compile(r"([A-Za-z_][\w\s*]*?)\b(mgf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _ctype(decl, proto, result=False):
    words = decl.replace("*", " * ").split()
    plain = [w for w in words if w != "const"]
    if result and plain == ["void"]:
        return None
    if "*" in plain:
        if not result:
            return vp
        if words == ["const", "char", "*"]:
            return C.c_char_p
    elif plain and plain[0] in _SCALARS and (len(plain) == 1 or (len(plain) == 2 and not result and plain[1].isidentifier())):
        return _SCALARS[plain[0]]
    raise MgfError(f"include/mgf.h: no binding rule for {' '.join(words)!r} in `{proto}`")


def parse_header(text):
    """(signatures, constants) of a C header in the dialect of include/mgf.h: `name -> (restype, [argtypes])` for every `mgf_*`
    prototype, and `NAME -> int` for every enumerator of an `enum { NAME = value, ... };` block and every `#define MGF_NAME <integer>`.
    Raises MgfError for what it does not understand (a type outside _SCALARS, an `mgf_*(` that is no plain prototype: a function-pointer
    parameter, a declaration inside a macro), so that no export drops out of the binding silently."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {name: int(value) for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MGF_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    for body in re.findall(r"\benum\s*\{([^{}]*)\}\s*;", text):
        for item in filter(None, map(str.strip, body.split(","))):
            m = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item)
            if not m:
                raise MgfError(f"include/mgf.h: enumerator `{item}` has no explicit decimal value")
            consts[m.group(1)] = int(m.group(2))
    sigs = {}
    for m in _PROTOTYPE.finditer(re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)):
        ret, name, params = m.groups()
        proto = " ".join(m.group(0).split())
        params = [] if params.split() in ([], ["void"]) else params.split(",")
        sigs[name] = (_ctype(ret, proto, result=True), [_ctype(p, proto) for p in params])
    unparsed = sorted(set(re.findall(r"\b(mgf_[a-z0-9_]+)\s*\(", text)) - set(sigs))
    if unparsed:
        raise MgfError(f"include/mgf.h: {', '.join(unparsed)}: not a plain prototype `type mgf_name(type arg, ...);`, cannot be bound")
    return sigs, consts


try:
    with open(HEADER_PATH) as _f:
        _SIGS, CONSTANTS = parse_header(_f.read())
except OSError as e:
    raise MgfError(f"{HEADER_PATH}: the C header the binding is read from is missing ({e}); the package is used in place, in its tree") from None
globals().update(CONSTANTS)           # MGF_OK / MGF_E*, MGF_F32 / MGF_F64 / MGF_F16, MGF_ACT_*, MGF_FILTER_*, MGF_CROP_*, MGF_MAX_TAPS
EXPORTED_SYMBOLS = sorted(_SIGS)
MAX_TAPS = CONSTANTS["MGF_MAX_TAPS"]
ACT_IDS = {name[len("MGF_ACT_"):].lower(): value for name, value in CONSTANTS.items() if name.startswith("MGF_ACT_")}


class Epilogue(C.Structure):
    _fields_ = [("bias", vp), ("noise", vp), ("noise_strength", vp), ("noise_n", i32), ("act", i32), ("alpha", f32),
                ("gain", f32), ("residual", vp)]


class ConvDesc(C.Structure):
    _fields_ = [("n", i32), ("cin", i32), ("in_h", i32), ("in_w", i32), ("cout", i32), ("cout_pad", i32),
                ("tile_h", i32), ("tile_w", i32), ("istride", i32), ("ostride", i32), ("ntaps", i32), ("ngroups", i32),
                ("dy", i32 * MAX_TAPS), ("dx", i32 * MAX_TAPS), ("group", i32 * MAX_TAPS), ("oy", i32 * 4), ("ox", i32 * 4),
                ("out_h", i32), ("out_w", i32), ("y_pitch", i64), ("y_plane", i64), ("y_batch", i64), ("y_choff", i32),
                ("out_scale_stride", i32), ("workspace", vp), ("workspace_floats", i64),
                ("rgb_w", vp), ("rgb_bias", vp), ("rgb_out", vp), ("rgb_channels", i32), ("pad_", i32)]


class ConvProfRec(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("flops", f64), ("seconds", f64), ("bytes", f64), ("ksplit", i32), ("pad_", i32)]


class StyleJob(C.Structure):
    _fields_ = [("aff_w", vp), ("aff_b", vp), ("wsq", vp), ("s", vp), ("d", vp), ("cin", i32), ("cout", i32),
                ("w_offset", i32), ("aff_gain", f32), ("style_gain", f32)]


class AttnJob(C.Structure):
    _fields_ = [("wmv", vp), ("bmv", vp), ("vwb", vp), ("c", i32), ("w_offset", i32)]


class StyleBwdJob(C.Structure):
    _fields_ = [("aff_w", vp), ("wsq", vp), ("s", vp), ("d", vp), ("ds_part", vp), ("dc_part", vp), ("cin", i32), ("cout", i32),
                ("s_chunks", i32), ("d_chunks", i32), ("aff_gain", f32), ("style_gain", f32)]


class AttnGradJob(C.Structure):
    _fields_ = [("dg", vp), ("probs", vp), ("dc", vp), ("cpre", vp), ("part", vp), ("dvwb", vp), ("dc_part", vp), ("c", i32), ("f", i32),
                ("slices", i32), ("nchunk", i32), ("blk_grad", i32), ("blk_dot", i32), ("blk_red", i32), ("pad_", i32)]


class AttnBwdJob(C.Structure):
    _fields_ = [("wmv", vp), ("dvwb", vp), ("c", i32), ("pad_", i32)]


_lib = None


def lib() -> C.CDLL:
    """Load libmgf_hip.so (once).  Raises if it has not been built -- never falls back."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MgfError(f"{LIB_PATH} is missing: run `python -m morphganformer_amd.build` (or __graft_entry__.build()). "
                           "There is no CPU fallback for the HIP path.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().mgf_last_error().decode(errors="replace")
        raise MgfError(f"{what or 'mgf'} failed (code {rc}): {msg}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def map_table(sides, offsets):
    """The host-side map table of the mgf_noise_sets_* entries: (sides as int32[n], offsets as int64[n], n)."""
    n = len(sides)
    assert len(offsets) == n
    return (i32 * n)(*[int(s) for s in sides]), (i64 * n)(*[int(o) for o in offsets]), n


def device_table(arr, device):
    """A ctypes array of job records as a uint8 tensor on `device`: the `*_jobs_dev` argument of the batched entries."""
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise MgfError(f"HIP op received a tensor on '{t.device}'; the MI355X path has no CPU fallback "
                           "(use impl='ref' only in oracle tests)")


def dtype_id(dt: torch.dtype) -> int:
    try:
        return {torch.float32: MGF_F32, torch.float64: MGF_F64, torch.float16: MGF_F16}[dt]
    except KeyError:
        raise MgfError(f"unsupported dtype {dt}") from None


def make_epilogue(bias=None, noise=None, noise_strength=None, noise_n=1, act="linear", alpha=0.2, gain=1.0, residual=None):
    ep = Epilogue(ptr(bias), ptr(noise), ptr(noise_strength), int(noise_n), ACT_IDS[act], float(alpha), float(gain),
                  ptr(residual))
    # the struct holds raw device pointers: keep the tensors alive as long as it lives, so that a temporary passed by the caller
    # (`make_epilogue(bias=b.cuda())`) is not handed back to the caching allocator -- and reused for the launch's own output -- before
    # the kernel that reads it has been enqueued (after that the allocator's stream ordering protects it)
    ep._keep = (bias, noise, noise_strength, residual)
    return ep
