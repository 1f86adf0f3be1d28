"""The MDF objective (multi-scale discriminative feature loss, mdfloss.py:16-47) on MI355X: SinGAN WDiscriminators
(SinGAN/models.py:7-35) as fixed loss networks.

    D(x) = [x1, x2, x3]:  x1 = lrelu(BN(conv(x)))            head, 3 -> N        (all convs 3x3, stride 1, padding 0)
                          x2 = 3 x lrelu(BN(conv(.)))(x1)    body, N -> N
                          x3 = conv(x2)                      tail, N -> 1
    loss[b] = sum over the selected discriminators D, in order, and the taps t of mean((D(x)_t - D(y)_t)^2)

The weight files (mdf-main/weights/Ds_{SISR,Denoising,JPEG}.pth) are pickled lists of whole modules: `load_discriminators` reads them
with a restricted unpickler (nothing from the file is imported or executed) into per-discriminator state dicts, checks the architecture
the kernels assume and refuses anything else.  Eval-mode BatchNorm is folded into each conv once, in float64.  The kernels
(csrc/mdf.hip) work on frames of the image's size -- see include/mgf.h, "MDF objective".
"""
from __future__ import annotations

import collections
import io
import math
import os
import pickle
import struct
import zipfile

import numpy as np
import torch

from . import _lib
from . import conv as cv

BN_EPS = 1e-5
SLOPE = 0.2
WIDTHS = (32, 64, 128)
BODY_BLOCKS = 3
RING_X2 = 1 + BODY_BLOCKS            # ring depth of x2 in the frame (include/mgf.h)
MIN_SIDE = 2 * (RING_X2 + 1) + 1     # 11: the smallest image with one x3 value
_CONVS = ["head.conv"] + [f"body.block{i + 1}.conv" for i in range(BODY_BLOCKS)]
_NORMS = ["head.norm"] + [f"body.block{i + 1}.norm" for i in range(BODY_BLOCKS)]


# ------------------------------------------------------------------------------------------------------------------ weight files
class _Inert:
    """Stand-in for a pickled module class: keeps the pickled state, has no behaviour."""
    _kind = "?"

    def __setstate__(self, state):
        self.__dict__.update(state if isinstance(state, dict) else {"_state": state})


def _inert(kind):
    return type(kind, (_Inert,), {"_kind": kind})


_STANDINS = {("SinGAN.models", "WDiscriminator"): _inert("WDiscriminator"), ("SinGAN.models", "ConvBlock"): _inert("ConvBlock"),
             ("torch.nn.modules.conv", "Conv2d"): _inert("Conv2d"), ("torch.nn.modules.batchnorm", "BatchNorm2d"): _inert("BatchNorm2d"),
             ("torch.nn.modules.activation", "LeakyReLU"): _inert("LeakyReLU"),
             ("torch.nn.modules.container", "Sequential"): _inert("Sequential")}


class _StorageType:
    def __init__(self, dtype):
        self.dtype = dtype


class _Storage:
    def __init__(self, key, dtype, numel):
        self.key, self.dtype, self.numel, self.data = key, dtype, int(numel), None


class _TensorRef:
    def __init__(self, storage, offset, size, stride):
        self.storage, self.offset, self.size, self.stride = storage, int(offset), tuple(size), tuple(stride)

    def tensor(self):
        if self.storage.data is None:
            raise _lib.MgfError(f"MDF weights: storage {self.storage.key!r} has no data in the file")
        return torch.as_strided(self.storage.data, self.size, self.stride, self.offset).clone()


def _rebuild_tensor_v2(storage, storage_offset, size, stride, requires_grad=False, backward_hooks=None, metadata=None):
    return _TensorRef(storage, storage_offset, size, stride)


def _rebuild_parameter(data, requires_grad=False, backward_hooks=None):
    return data


_FUNCS = {("collections", "OrderedDict"): collections.OrderedDict, ("builtins", "set"): set, ("__builtin__", "set"): set,   # (a module's
          # _non_persistent_buffers_set in files of newer torch)
          ("torch._utils", "_rebuild_tensor_v2"): _rebuild_tensor_v2, ("torch._utils", "_rebuild_parameter"): _rebuild_parameter,
          ("torch", "FloatStorage"): _StorageType(torch.float32), ("torch", "LongStorage"): _StorageType(torch.int64)}


class _Unpickler(pickle.Unpickler):
    """Resolves only the globals of a SinGAN discriminator list (inert stand-ins for the module classes); refuses everything else
    before anything could run.  Storages are collected by key (their bytes follow the pickle, or sit in the zip archive)."""

    def __init__(self, f, storages=None):
        super().__init__(f)
        self.storages = storages

    def find_class(self, module, name):
        obj = _STANDINS.get((module, name)) or _FUNCS.get((module, name))
        if obj is None:
            raise _lib.MgfError(f"MDF weights: refusing to resolve global {module}.{name} (not a SinGAN discriminator list)")
        return obj

    def persistent_load(self, pid):
        if self.storages is None or not isinstance(pid, tuple) or not pid:
            raise _lib.MgfError("MDF weights: unexpected persistent id")
        kind = pid[0].decode() if isinstance(pid[0], bytes) else pid[0]
        if kind == "module":                       # legacy format: (module, class, source file, source text) -- the text is ignored
            if not (isinstance(pid[1], type) and issubclass(pid[1], _Inert)):
                raise _lib.MgfError("MDF weights: a module record names a class outside the allow-list")
            return pid[1]
        if kind != "storage" or not isinstance(pid[1], _StorageType):
            raise _lib.MgfError(f"MDF weights: unsupported persistent record {kind!r}")
        key, numel = str(pid[2]), int(pid[4])
        if len(pid) > 5 and pid[5] is not None:
            raise _lib.MgfError("MDF weights: storage views are not supported")
        st = self.storages.get(key)
        if st is None:
            st = self.storages[key] = _Storage(key, pid[1].dtype, numel)
        return st


def _read_legacy(f):
    for _ in range(3):                             # magic number, protocol version, system info: plain data
        _Unpickler(f).load()
    storages = {}
    obj = _Unpickler(f, storages).load()
    keys = _Unpickler(f).load()
    for key in keys:
        st = storages[str(key)]
        numel = struct.unpack("<q", f.read(8))[0]
        es = torch.empty((), dtype=st.dtype).element_size()
        raw = f.read(numel * es)
        if len(raw) != numel * es:
            raise _lib.MgfError("MDF weights: truncated storage data")
        st.data = _from_bytes(raw, st.dtype)
    return obj


def _from_bytes(raw, dtype):
    return torch.frombuffer(bytearray(raw), dtype=dtype) if raw else torch.empty(0, dtype=dtype)


def _read_zip(path):
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
        pkl = [n for n in names if n.endswith("/data.pkl") or n == "data.pkl"]
        if len(pkl) != 1:
            raise _lib.MgfError("MDF weights: zip archive without one data.pkl")
        root = pkl[0][:-len("data.pkl")]
        storages = {}
        obj = _Unpickler(io.BytesIO(z.read(pkl[0])), storages).load()
        for key, st in storages.items():
            raw = z.read(f"{root}data/{key}")
            st.data = _from_bytes(raw, st.dtype)
    return obj


def _children(m):
    return m.__dict__.get("_modules", {}) or {}


def _tensors(m, prefix, out):
    for group in ("_parameters", "_buffers"):
        for k, v in (m.__dict__.get(group, {}) or {}).items():
            if v is not None:
                out[prefix + k] = v.tensor().numpy() if isinstance(v, _TensorRef) else np.asarray(v)


def _expect(cond, what):
    if not cond:
        raise _lib.MgfError(f"MDF weights: {what} (the kernels implement SinGAN's WDiscriminator: 3x3 / stride-1 / padding-0 convs, "
                            f"eval-mode BatchNorm, LeakyReLU({SLOPE}), {BODY_BLOCKS} body blocks, N in {WIDTHS})")


def _check_conv(m, name):
    _expect(getattr(m, "_kind", None) == "Conv2d", f"{name} is not a Conv2d")
    d = m.__dict__
    _expect(tuple(d.get("kernel_size", ())) == (3, 3) and tuple(d.get("stride", ())) == (1, 1), f"{name}: kernel / stride")
    _expect(tuple(d.get("padding", ())) in ((0, 0),) and tuple(d.get("dilation", (1, 1))) == (1, 1) and d.get("groups", 1) == 1,
            f"{name}: padding / dilation / groups")


def _module_to_state(D, idx):
    """One pickled WDiscriminator stand-in -> (state dict of numpy arrays, BatchNorm eps)."""
    _expect(getattr(D, "_kind", None) == "WDiscriminator", f"entry {idx} is not a WDiscriminator")
    top = _children(D)
    _expect(set(top) == {"head", "body", "tail"}, f"entry {idx}: modules {sorted(top)}")
    body = _children(top["body"])
    _expect(list(body) == [f"block{i + 1}" for i in range(BODY_BLOCKS)], f"entry {idx}: body blocks {list(body)}")
    sd, eps = {}, None
    for prefix, blk in [("head", top["head"])] + [(f"body.{k}", v) for k, v in body.items()]:
        parts = _children(blk)
        _expect(getattr(blk, "_kind", None) == "ConvBlock" and list(parts) == ["conv", "norm", "LeakyRelu"], f"entry {idx}: {prefix}")
        _check_conv(parts["conv"], f"entry {idx} {prefix}.conv")
        bn, act = parts["norm"].__dict__, parts["LeakyRelu"].__dict__
        _expect(getattr(parts["norm"], "_kind", None) == "BatchNorm2d" and bn.get("affine", True) and bn.get("track_running_stats", True),
                f"entry {idx}: {prefix}.norm")
        _expect(not bn.get("training", False) and not D.__dict__.get("training", False), f"entry {idx} is in training mode")
        _expect(eps is None or eps == float(bn["eps"]), f"entry {idx}: mixed BatchNorm eps")
        eps = float(bn["eps"])
        _expect(getattr(parts["LeakyRelu"], "_kind", None) == "LeakyReLU" and abs(float(act.get("negative_slope", -1)) - SLOPE) < 1e-12,
                f"entry {idx}: {prefix} activation")
        _tensors(parts["conv"], prefix + ".conv.", sd)
        _tensors(parts["norm"], prefix + ".norm.", sd)
    _check_conv(top["tail"], f"entry {idx} tail")
    _tensors(top["tail"], "tail.", sd)
    return sd, eps


def check_state(sd, idx=0):
    """Shape checks of one discriminator's state dict; returns its width N."""
    g = lambda k: np.asarray(sd[k]) if k in sd else None
    w0 = g("head.conv.weight")
    _expect(w0 is not None and w0.ndim == 4 and w0.shape[1:] == (3, 3, 3), f"entry {idx}: head.conv.weight")
    N = int(w0.shape[0])
    _expect(N in WIDTHS, f"entry {idx}: width {N}")
    for c, nrm in zip(_CONVS, _NORMS):
        cin = 3 if c == "head.conv" else N
        _expect(g(c + ".weight") is not None and g(c + ".weight").shape == (N, cin, 3, 3), f"entry {idx}: {c}.weight")
        _expect(g(c + ".bias") is not None and g(c + ".bias").shape == (N,), f"entry {idx}: {c}.bias")
        for k in ("weight", "bias", "running_mean", "running_var"):
            _expect(g(f"{nrm}.{k}") is not None and g(f"{nrm}.{k}").shape == (N,), f"entry {idx}: {nrm}.{k}")
    _expect(g("tail.weight") is not None and g("tail.weight").shape == (1, N, 3, 3), f"entry {idx}: tail.weight")
    _expect(g("tail.bias") is not None and g("tail.bias").shape == (1,), f"entry {idx}: tail.bias")
    return N


def load_discriminators(path, device="cpu"):
    """Read a Ds_*.pth file (legacy or zip torch serialization of a list of WDiscriminator modules, or of per-discriminator state
    dicts) without importing or executing anything from it.  Returns a list of state dicts (torch float32 tensors on `device`; the
    files' cuda:0 storages are remapped) with an "eps" entry (BatchNorm eps, a float)."""
    if zipfile.is_zipfile(path):
        obj = _read_zip(path)
    else:
        with open(path, "rb") as f:
            obj = _read_legacy(f)
    if not isinstance(obj, (list, tuple)) or not obj:
        raise _lib.MgfError("MDF weights: the file does not hold a list of discriminators")
    out = []
    for i, D in enumerate(obj):
        if isinstance(D, dict):
            sd = {k: (v.tensor().numpy() if isinstance(v, _TensorRef) else np.asarray(v)) for k, v in D.items()}
            eps = BN_EPS
        else:
            sd, eps = _module_to_state(D, i)
        check_state(sd, i)
        entry = {k: torch.as_tensor(np.array(v, dtype=np.float32), device=device) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
        entry["eps"] = float(eps)
        out.append(entry)
    return out


def random_discriminators(seed=0, nfc=(32,) * 4 + (64,) * 4):
    """Seeded discriminators for tests and smoke runs: one state dict (numpy float32) per width in `nfc`, He-scaled convs,
    BatchNorm with non-trivial affine and running statistics.  numpy's default_rng: every machine draws the same values."""
    rng = np.random.default_rng(seed)
    out = []
    for N in nfc:
        sd = {}
        for c, nrm in zip(_CONVS, _NORMS):
            cin = 3 if c == "head.conv" else N
            sd[c + ".weight"] = (rng.standard_normal((N, cin, 3, 3)) * math.sqrt(2.0 / (9 * cin))).astype(np.float32)
            sd[c + ".bias"] = (rng.standard_normal(N) * 0.05).astype(np.float32)
            sd[nrm + ".weight"] = rng.uniform(0.5, 1.5, N).astype(np.float32)
            sd[nrm + ".bias"] = (rng.standard_normal(N) * 0.1).astype(np.float32)
            sd[nrm + ".running_mean"] = (rng.standard_normal(N) * 0.1).astype(np.float32)
            sd[nrm + ".running_var"] = rng.uniform(0.5, 1.5, N).astype(np.float32)
        sd["tail.weight"] = (rng.standard_normal((1, N, 3, 3)) * math.sqrt(1.0 / (9 * N))).astype(np.float32)
        sd["tail.bias"] = (rng.standard_normal(1) * 0.05).astype(np.float32)
        out.append(sd)
    return out


def _f64(v):
    return v.detach().cpu().double().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)


def fold_bn(sd, eps=BN_EPS):
    """Eval-mode BatchNorm folded into the convs, in float64: w' = w g / sqrt(rv + eps), b' = (b - rm) g / sqrt(rv + eps) + beta.
    Returns [(w', b')] for head, body blocks and tail (float64 numpy; the tail has no norm)."""
    eps = float(sd.get("eps", eps)) if isinstance(sd, dict) else eps
    layers = []
    for c, nrm in zip(_CONVS, _NORMS):
        s = _f64(sd[nrm + ".weight"]) / np.sqrt(_f64(sd[nrm + ".running_var"]) + eps)
        layers.append((_f64(sd[c + ".weight"]) * s[:, None, None, None], (_f64(sd[c + ".bias"]) - _f64(sd[nrm + ".running_mean"])) * s
                       + _f64(sd[nrm + ".bias"])))
    layers.append((_f64(sd["tail.weight"]), _f64(sd["tail.bias"])))
    return layers


def adjoint_weights(w):
    """The adjoint of a 3x3 pad-1 convolution as another one: W~[ci][co][kh][kw] = W[co][ci][2-kh][2-kw] (float64 numpy; transposing and
    flipping is exact, so its float32 rounding is the transposed rounding of W)."""
    w = np.asarray(w, dtype=np.float64)
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


class _Disc:
    """One discriminator's folded weights on the device, in the layouts of the mdf kernels."""

    def __init__(self, sd, device, idx, differentiable=False):
        self.N = check_state(sd, idx)
        layers = fold_bn(sd)
        t32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=device)
        (hw, hb), body, (tw, tb) = layers[0], layers[1:-1], layers[-1]
        self.head_w, self.head_b = t32(hw.reshape(self.N, 27)), t32(hb)
        self.body_w = [t32(w) for w, _ in body]
        self.body_b = [t32(b) for _, b in body]
        self.body_u = [cv.winograd2_weights(w) for w in self.body_w]
        self.tail_w, self.tail_b = t32(tw.reshape(self.N * 9)), float(np.float32(tb[0]))
        # backward: the body blocks' adjoints as Winograd weight planes (the head and tail backward kernels read head_w / tail_w flipped)
        self.body_uadj = [cv.winograd2_weights(t32(adjoint_weights(w))) for w, _ in body] if differentiable else None
        self._packed = None

    def packed(self):
        """Tap-list weights of the body (MGF_MDF_BODY=taps: the A/B reference path of tools/mdf_bench.py)."""
        if self._packed is None:
            self._packed = [cv.pack_weights(w) for w in self.body_w]
        return self._packed


def _body_on_taps():
    return os.environ.get("MGF_MDF_BODY", "winograd") == "taps"      # tuning hook: the body on the direct tap-list kernel


class MDFLoss:
    """loss[i] = sum over the selected discriminators and their three taps of mean((D(pred[i])_t - D(target)_t)^2)
    (mdfloss.py:16-47 for one candidate; `forward` / `__call__` add the reference's batch mean).  The target's taps are computed once
    per target (the reference recomputes them every step)."""

    def __init__(self, Ds, num_scales=8, is_ascending=1, device="cuda", differentiable=False):
        """Ds: a Ds_*.pth path or a list of per-discriminator state dicts (load_discriminators / random_discriminators).
        num_scales discriminators are used, Ds[0 ..] ascending or Ds[-1 ..] descending (mdfloss.py:24-31).
        differentiable: also build the backward pass (distance_into(dimg=...), autograd through `forward`, GradientProjectionEngine): the
        adjoint weights are prepared once and the workspace keeps one discriminator's activations x1, a1, a2, x2 (4 N planes) and x3 per
        candidate.  Without it memory and launches are those of the literal loop."""
        _lib.lib()
        self.device = torch.device(device)
        if isinstance(Ds, (str, bytes, os.PathLike)):
            Ds = load_discriminators(Ds)
        self.num_discs = len(Ds)
        if not 1 <= int(num_scales) <= self.num_discs:
            raise _lib.MgfError(f"MDFLoss: num_scales must be 1 .. {self.num_discs} (the file holds {self.num_discs} discriminators)")
        self.num_scales, self.is_ascending = int(num_scales), int(is_ascending)
        self.order = [s if self.is_ascending else self.num_discs - 1 - s for s in range(self.num_scales)]
        self.differentiable = bool(differentiable)
        self.nets = [_Disc(Ds[i], self.device, i, self.differentiable) for i in self.order]
        self.cmax = max(d.N for d in self.nets)
        self._hw, self._n = None, 0
        self._tgt = None

    # ------------------------------------------------------------------ workspace
    def _reserve(self, n, h, w):
        if (h, w) != self._hw or n > self._n:
            if h < MIN_SIDE or w < MIN_SIDE:
                raise _lib.MgfError(f"MDFLoss: images of at least {MIN_SIDE}x{MIN_SIDE} pixels (got {h}x{w}): five valid 3x3 convolutions")
            e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=self.device)
            self.frames = [e(n * self.cmax * h * w), e(n * self.cmax * h * w)]     # (differentiable: also the two gradient frames)
            if self.differentiable:                                                # x1, a1, a2, x2 and x3 of the discriminator in flight
                self.acts = [e(n * self.cmax * h * w) for _ in range(1 + BODY_BLOCKS)]
                self.x3 = e(n * h * w)
            self.nblk = int(_lib.lib().mgf_mdf_partials(h, w))
            self.part = e(3 * len(self.nets), n, self.nblk, dt=torch.float64)
            self._hw, self._n = (h, w), n
            counts = []
            for d in self.nets:
                counts += [d.N * (h - 2) * (w - 2), d.N * (h - 2 * RING_X2) * (w - 2 * RING_X2), (h - 2 * RING_X2 - 2) * (w - 2 * RING_X2 - 2)]
            self.counts = (_lib.f64 * len(counts))(*counts)

    def _body(self, d, x, y, n, h, w, k):
        if _body_on_taps():
            per = d.N * h * w                                  # (the workspace frames are sized for the widest D)
            step = max(1, (2 ** 31 - 1) // per)                # the tap-list launch takes < 2^31 input elements
            for s in range(0, n, step):
                k1 = min(n, s + step)
                m = lambda t: t.reshape(-1)[s * per:k1 * per].view(k1 - s, d.N, h, w)
                cv.conv_forward(m(x), d.packed()[k], pad=(1, 1), epilogue=_lib.make_epilogue(bias=d.body_b[k], act="lrelu", alpha=SLOPE),
                                out=m(y))
            return
        _lib.check(_lib.lib().mgf_mdf_body_f32(y.data_ptr(), x.data_ptr(), d.body_u[k].data_ptr(), d.body_b[k].data_ptr(), n, d.N, h, w,
                                               SLOPE, _lib.stream_ptr()), "mdf_body")

    def _features(self, d, img, n, h, w, x1, x2_out, x3_out, tgt=None, part=None, mids=None):
        """head -> 3 body blocks -> tail of one discriminator on img [n,3,h,w].  With tgt = (x1t, x2t, x3t) and part (3 slabs) the taps'
        partial sums land in part; without, the taps are written to x1 / x2_out / x3_out (the target's frames).  mids: frames for a1 and
        a2 (the backward keeps them) instead of the workspace's ping-pong."""
        L, st = _lib.lib(), _lib.stream_ptr()
        _lib.check(L.mgf_mdf_head_f32(x1.data_ptr(), _lib.ptr(part[0] if part is not None else None), img.data_ptr(), d.head_w.data_ptr(),
                                      d.head_b.data_ptr(), _lib.ptr(tgt[0] if tgt else None), n, d.N, h, w, SLOPE, st), "mdf_head")
        f0, f1 = self.frames
        # ping-pong through the two workspace frames; the target's x1 / x2 land in its own frames
        seq = [x1, f0, f1, x2_out] if x2_out is not None else [x1, f1, f0, f1]
        if mids is not None:
            seq = [x1, mids[0], mids[1], x2_out]
        for k in range(BODY_BLOCKS):
            self._body(d, seq[k], seq[k + 1], n, h, w, k)
        x2 = seq[BODY_BLOCKS]
        _lib.check(L.mgf_mdf_tail_f32(_lib.ptr(x3_out), _lib.ptr(part[1] if part is not None else None),
                                      _lib.ptr(part[2] if part is not None else None), x2.data_ptr(), d.tail_w.data_ptr(), d.tail_b,
                                      _lib.ptr(tgt[1] if tgt else None), _lib.ptr(tgt[2] if tgt else None), n, d.N, h, w, RING_X2, st),
                   "mdf_tail")

    # ------------------------------------------------------------------ public
    def set_target(self, target):
        """target [1,3,H,W] in [-1, 1].  The taps of every selected discriminator are kept on the device (frames: 2 N + 1 planes of
        H x W per discriminator); with the same shape they are rewritten IN PLACE -- a captured hipGraph keeps reading them."""
        _lib.require_gpu(target)
        if target.dim() != 4 or target.shape[0] != 1 or target.shape[1] != 3:
            raise _lib.MgfError(f"MDFLoss.set_target: one [1, 3, H, W] image (got {tuple(target.shape)})")
        h, w = int(target.shape[2]), int(target.shape[3])
        self._reserve(max(self._n, 1), h, w)
        img = target.detach().float().contiguous()
        if self._tgt is None or self._tgt_hw != (h, w):
            e = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
            self._tgt = [(e(d.N, h, w), e(d.N, h, w), e(h, w)) for d in self.nets]
            self._tgt_hw = (h, w)
        for d, (x1t, x2t, x3t) in zip(self.nets, self._tgt):
            self._features(d, img, 1, h, w, x1t, x2t, x3t)

    def _backward(self, i, d, tgt, dimg, n, h, w, scale, accumulate):
        """dimg (+)= scale * d loss_i / d pred for discriminator position i, from the activations its forward left in self.acts / self.x3
        (include/mgf.h, "MDF backward"): tail -> three masked body adjoints -> head, through the two gradient frames."""
        L, st = _lib.lib(), _lib.stream_ptr()
        A, (g0, g1) = self.acts, self.frames
        c1, c2, c3 = (float(self.counts[3 * i + t]) for t in range(3))
        _lib.check(L.mgf_mdf_tail_backward_f32(g0.data_ptr(), A[3].data_ptr(), tgt[1].data_ptr(), self.x3.data_ptr(), tgt[2].data_ptr(),
                                               d.tail_w.data_ptr(), n, d.N, h, w, RING_X2, 2.0 * scale / c2, 2.0 * scale / c3, SLOPE, st),
                   "mdf_tail_backward")
        src, dst = g0, g1
        for k in reversed(range(BODY_BLOCKS)):           # delta_k = adj_{k+1}(delta_{k+1}) * phi'(a_k) on ring k + 1
            _lib.check(L.mgf_mdf_body_backward_f32(dst.data_ptr(), src.data_ptr(), d.body_uadj[k].data_ptr(), A[k].data_ptr(), n, d.N, h, w,
                                                   k + 1, SLOPE, st), "mdf_body_backward")
            src, dst = dst, src
        _lib.check(L.mgf_mdf_head_backward_f32(dimg.data_ptr(), src.data_ptr(), A[0].data_ptr(), tgt[0].data_ptr(), d.head_w.data_ptr(), n, d.N,
                                               h, w, 2.0 * scale / c1, SLOPE, int(accumulate), st), "mdf_head_backward")

    def _run(self, pred, dimg=None, scale=1.0, grad_accumulate=False):
        assert self._tgt is not None, "call set_target first"
        _lib.require_gpu(pred)
        n, c, h, w = pred.shape
        if c != 3 or (h, w) != self._tgt_hw:
            raise _lib.MgfError(f"MDFLoss: candidates must be [n, 3, {self._tgt_hw[0]}, {self._tgt_hw[1]}] like the target (got {tuple(pred.shape)})")
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            raise _lib.MgfError("MDFLoss: candidates must be contiguous float32")
        self._reserve(n, h, w)
        part = self.part_view(n)
        for i, (d, tgt) in enumerate(zip(self.nets, self._tgt)):
            slabs = [part[3 * i + t] for t in range(3)]
            if dimg is None:
                self._features(d, pred, n, h, w, self.frames[0], None, None, tgt, slabs)
            else:                                        # forward keeping the activations, then this discriminator's backward
                A = self.acts
                self._features(d, pred, n, h, w, A[0], A[3], self.x3, tgt, slabs, mids=(A[1], A[2]))
                self._backward(i, d, tgt, dimg, n, h, w, scale, grad_accumulate or i > 0)
        return part, n

    def part_view(self, n):
        """The slabs of an n-candidate call laid out [3 S][n][nblk] (contiguous: the finish kernel's layout)."""
        need = 3 * len(self.nets) * n * self.nblk
        return self.part.view(-1)[:need].view(3 * len(self.nets), n, self.nblk)

    def distance_into(self, out, pred, scale=1.0, accumulate=False, dimg=None, grad_accumulate=False):
        """out[i] (+)= scale * loss(pred[i]);  out: float32 [n].  Graph-capturable once a call of this batch size has run (workspace).
        dimg (differentiable=True): also dimg[i] (+)= scale * d loss(pred[i]) / d pred[i] (grad_accumulate: +=), each discriminator's
        backward right behind its own forward; the loss is the same bits as without dimg, a candidate's gradient the same bits in any batch."""
        if dimg is not None:
            if not self.differentiable:
                raise _lib.MgfError("MDFLoss.distance_into(dimg=...): build the loss with MDFLoss(..., differentiable=True) for its backward pass")
            if tuple(dimg.shape) != tuple(pred.shape) or dimg.dtype != torch.float32 or not dimg.is_contiguous():
                raise _lib.MgfError(f"MDFLoss: dimg must be a contiguous float32 tensor shaped like pred {tuple(pred.shape)}")
        part, n = self._run(pred, dimg, float(scale), grad_accumulate)
        _lib.check(_lib.lib().mgf_mdf_finish_f32(out.data_ptr(), part.data_ptr(), part.shape[0], self.nblk, self.counts, n, float(scale),
                                                 int(accumulate), _lib.stream_ptr()), "mdf_finish")
        return out

    def distance_per_tap(self, pred):
        """float64 [n, num_scales, 3]: mean((D(pred[i])_t - D(target)_t)^2) per discriminator position and tap (host-side sums of the
        kernels' partial slabs; tests)."""
        part, n = self._run(pred)
        sums = part.sum(dim=2).double().cpu().numpy()                # [3 S, n]
        counts = np.array(list(self.counts), dtype=np.float64)
        return torch.from_numpy((sums / counts[:, None]).T.reshape(n, len(self.nets), 3).copy())

    def forward(self, x, y):
        """The reference's call: mean over the batch of loss(x[i], y[i]) (mdfloss.py:16-47; x = the target(s), y = the candidates).
        differentiable=True and y.requires_grad: the result is connected to y (the gradient is computed here, eagerly, and scaled by
        grad_output / n in backward) -- the reference's `p_loss = criterion(imgs, img_gen); p_loss.backward()`.  Otherwise detached."""
        if self.differentiable and y.requires_grad and torch.is_grad_enabled():
            return _MDFFunction.apply(y, self, x)
        return self._forward_detached(x, y)[0]

    def _forward_detached(self, x, y, want_grad=False):
        y = y.detach().float().contiguous()
        g = torch.empty_like(y) if want_grad else None
        out = torch.zeros(y.shape[0], dtype=torch.float32, device=y.device)
        if x.shape[0] == 1:
            self.set_target(x)
            self.distance_into(out, y, dimg=g)
        else:
            assert x.shape[0] == y.shape[0], "x and y pair up"
            for i in range(x.shape[0]):
                self.set_target(x[i:i + 1])
                self.distance_into(out[i:i + 1], y[i:i + 1], dimg=None if g is None else g[i:i + 1])
        return out.mean(), g

    __call__ = forward


class _MDFFunction(torch.autograd.Function):
    """MDFLoss.forward with a gradient for the candidates: computed eagerly by the HIP backward, scaled in backward."""

    @staticmethod
    def forward(ctx, y, crit, x):
        loss, g = crit._forward_detached(x.detach(), y, want_grad=True)
        ctx.save_for_backward(g)
        ctx.n, ctx.dtype = int(y.shape[0]), y.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        g, = ctx.saved_tensors
        return (g * (grad_out / ctx.n)).to(ctx.dtype), None, None
