"""Record-and-replay gate for the convolution launches: recorder, sampled float64 evaluator, element selection, comparator.

Everything in the product reaches the convolution kernels through seven wrappers of morphganformer_amd/conv.py, looked up as module
attributes.  `Recorder` replaces them with shims that note WHAT was called (shapes and options, no tensors), `build_call` rebuilds one
such call on seeded random data -- same shapes, same options, so the dispatcher makes the same choice -- and `evaluate` gives the exact
value of that launch at a chosen set of output elements in float64 (gathered input patches contracted with torch.matmul; no
convolution routine of any library is involved).  `compare` is the gate:

    |got - ref64| <= c * A          per element,  A = sum |w| |x| over the element's own products (scales applied; + |bias| for a kernel
                                                  whose accumulator starts at the bias: Spec.bias_in_sum),
    c = max(m * r, sqrt(K) * 2^-24),  r = max |ref32 - ref64| / A over the launch's sampled elements,

where ref32 is the SAME evaluator run in float32 (the direct form in the arithmetic the kernels work in), K the products per output and
m = 4 for the tap-list, pointwise and narrow kernels (they differ from ref32 in summation order only, split-K included), m = 8 for the
Winograd forms (the F(2x2,3x3) transforms add a bounded constant).  The Winograd m started at 16 and proved slack; it was changed ONCE, to 8,
from the head-room max |got - ref64| / (r A) observed over every launch of every workload on an MI355X (profiles/conv_launch_census.txt):
form 3 one-shot 1.83, form 3 persistent 1.76, polyphase transposed conv 3.74 (up to 2.41 / 1.81 / 4.76 on three earlier seedings); against
their m = 4 tap-list 4.28 (under the sqrt(K) floor there: 0.51 c A), pointwise 3.59, few-outputs 2.98, few-inputs 2.38.  Beside the gate the
max-norm relative error of the sampled set stays within the bound the per-kernel test of that wrapper uses today (REL_BOUNDS).  m is never
tuned per launch; the data of a record is seeded by a hash of its own signature.

No pytest in here: tests/test_conv_replay_host.py, tests/test_hip_conv_replay.py and tools/conv_census.py import it.
"""
from __future__ import annotations

import inspect
import math
import zlib

import numpy as np
import torch

WRAPPERS = ("conv_forward", "winograd_forward", "winograd2_forward", "winograd2_rgb_forward", "tconv3x3s2_forward", "conv3x3_few_outputs",
            "conv3x3s2_few_inputs")
M_DIRECT, M_WINOGRAD = 4.0, 8.0
REL_BOUND = 2e-5                         # test_conv_taps_vs_torch, test_winograd_conv_matches_direct_conv_and_oracle, test_tconv_vs_torch, ...
# the max-norm bound of each replay is the one the per-kernel test of that launch uses (nothing weaker than today)
REL_BOUNDS = {"conv_forward": 2e-5,              # tests/test_hip_ops.py: test_conv_taps_vs_torch, test_conv1x1_register_gemm_vs_torch_and_tap_list
              "winograd_forward": 2e-5,          # test_winograd_conv_matches_direct_conv_and_oracle, test_winograd3_persistent_form
              "winograd2_forward": 2e-5,         # test_winograd_odd_maps_and_channel_slices
              "winograd2_rgb_forward": 2e-5,     # test_winograd_fused_torgb_matches_tap_list_launch
              "tconv3x3s2_forward": 2e-5,        # test_tconv_vs_torch, tests/test_hip_tconv_winograd.py
              "conv3x3s2_few_inputs": 2e-5,      # test_narrow_stride2_convs_vs_torch_and_tap_list
              "conv3x3_few_outputs": 5e-6,       # tests/test_hip_torgb_compose.py (its 1024^2 case included)
              "mdf_body": 1e-5,                  # tests/test_hip_mdf.py: test_body_kernel_against_float64_and_batch_invariant
              "mdf_body_backward": 2e-5}         # tests/test_hip_mdf_grad.py: _check_ring
CANARY = 12345.678
ACT_NAMES = {1: "linear", 2: "relu", 3: "lrelu", 10: "relu_post"}


class Unexpressible(Exception):
    """A record the evaluator cannot rebuild or evaluate: a test failure naming the record, never a silent skip."""


# ------------------------------------------------------------------------------------------------------------------ recorder
def _scale_sig(t):
    return None if t is None else (t.ndim, int(t.stride(0)) if t.ndim == 2 else 0, int(t.shape[0]))


def _ep_sig(ep):
    if ep is None:
        return None
    return (bool(ep.bias), bool(ep.noise), bool(ep.noise_strength), int(ep.noise_n), int(ep.act), round(float(ep.alpha), 7), round(float(ep.gain), 7),
            bool(ep.residual))


def _weight_sig(wobj):
    if isinstance(wobj, torch.Tensor):
        return ("tensor",) + tuple(wobj.shape)
    return ("packed", wobj.cout, wobj.cin, wobj.kh, wobj.kw, wobj.cout_pad)


def signature(name, fn, args, kwargs):
    """The hashable description of one wrapper call: everything the launch code can depend on, no tensor."""
    b = inspect.signature(fn).bind(*args, **kwargs)
    b.apply_defaults()
    a = b.arguments
    x = a["x"]
    sig = {"wrapper": name, "x": tuple(x.shape)}
    wobj = a.get("pc", a.get("u", a.get("w")))
    sig["weight"] = _weight_sig(wobj)
    sig["stride"] = int(a.get("stride", 1))
    sig["pad"] = tuple(a["pad"]) if "pad" in a else None
    sig["taps"] = tuple(tuple(t) for t in a["taps"]) if a.get("taps") is not None else None
    sig["ksize"] = tuple(a["ksize"]) if a.get("ksize") is not None else None
    sig["in_scale"] = _scale_sig(a.get("in_scale"))
    sig["out_scale"] = _scale_sig(a.get("out_scale"))
    sig["epilogue"] = _ep_sig(a.get("epilogue"))
    out = a.get("out", a.get("rgb_out"))
    sig["out"] = tuple(out.shape) if out is not None else None
    sig["out_choff"] = int(a.get("out_choff", 0))
    sig["residual_low"] = a.get("residual_low") is not None
    rgb = a.get("rgb")
    if name == "winograd2_rgb_forward":
        sig["rgb"] = (int(a["rgb_w"].shape[1]), a["rgb_bias"] is not None)
    else:
        sig["rgb"] = None if rgb is None else (int(rgb[0].shape[1]), rgb[1] is not None)
    sig["bf"] = a.get("bf") is not None
    sig["wt"] = a.get("wt") is not None
    sig["bias"] = a.get("bias") is not None              # the two narrow forms take bias / relu as plain arguments
    sig["relu"] = bool(a.get("relu", False))
    return tuple(sorted(sig.items()))


class Recorder:
    """with Recorder(cv) as rec: <workload>  ->  rec.records: {signature: launches}, launches = ((kernel name, ksplit), ...) of the call's
    own conv-profile bracket.  Outermost wrapper call only (winograd_forward delegating to winograd2_forward is one record).  A signature
    met again must launch what it launched the first time; anything else lands in rec.conflicts."""

    def __init__(self, cv, profile=True):
        self.cv, self.profile = cv, profile
        self.records, self.calls, self.conflicts = {}, 0, []
        self._depth, self._saved = 0, {}

    def _shim(self, name, fn):
        def shim(*args, **kwargs):
            if self._depth:
                return fn(*args, **kwargs)
            sig = signature(name, fn, args, kwargs)
            self._depth += 1
            try:
                if self.profile:
                    self.cv.profile_begin()
                try:
                    res = fn(*args, **kwargs)
                finally:
                    launches = tuple((r[0], r[3]) for r in self.cv.profile_end(64)) if self.profile else ()
            finally:
                self._depth -= 1
            self.calls += 1
            seen = self.records.setdefault(sig, launches)
            if seen != launches:
                self.conflicts.append((sig, seen, launches))
            return res
        return shim

    def __enter__(self):
        for name in WRAPPERS:
            self._saved[name] = getattr(self.cv, name)
            setattr(self.cv, name, self._shim(name, self._saved[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(self.cv, name, fn)
        self._saved = {}
        return False


# --------------------------------------------------------------------------------------------------------- element selection
def seam_indices(size, periods):
    """Both sides of every multiple of each period inside [0, size): m - 1 and m."""
    s = set()
    for p in periods:
        for m in range(p, size, p):
            s.update((m - 1, m))
    return sorted(i for i in s if 0 <= i < size)


def border_indices(size):
    return sorted({i for i in (0, 1, size - 2, size - 1) if 0 <= i < size})


def select_channels(cout, seed=0):
    """First, last and one interior channel of every 32-channel tile, plus every channel of the ragged tail."""
    rng = np.random.default_rng(seed)
    sel = set()
    for t0 in range(0, cout, 32):
        t1 = min(cout, t0 + 32)
        if t1 - t0 < 32:
            sel.update(range(t0, t1))
        else:
            sel.update((t0, t1 - 1, t0 + 1 + int(rng.integers(30))))
    return sorted(sel)


def select_samples(n):
    return sorted({0, min(1, n - 1), n - 1})


ROW_SEAMS, COL_SEAMS = (4, 8, 32), (16, 32)
STRIP_TILES = (4, 8, 16, 32)             # persistent form: a strip ends every 4 * L rows (vertical walk) or 32 * L columns (horizontal walk)


def select_positions(oh, ow, persistent=False, fill=2048, cross=8, seed=0):
    """(oy, ox) int64 arrays, no duplicates:
      * every element of the first and last two rows and columns;
      * both sides of every tile seam: rows at multiples of 4 / 8 / 32, columns at multiples of 16 / 32; a seam row is taken at EVERY seam and
        border column where it is also a seam of 16 rows (the 32-row tiles and every strip end of 4 / 8 / 16 / 32 tiles of 4 rows lie there),
        at `cross` seeded seam columns and every border column otherwise; with persistent=True the rows at both sides of every vertical
        strip end (multiples of 4 * L rows, L = 4 / 8 / 16 / 32) are taken at every seam column too.  Horizontal strip ends (every 32 * L columns)
        are multiples of 32 and so seam columns already: they are met at every border row and every row of a 16-row seam, and at the seeded
        subset of the other seam rows;
      * `fill` seeded random interior positions -- the only part a time budget may shrink."""
    rng = np.random.default_rng(seed)
    rows_b, cols_b = border_indices(oh), border_indices(ow)
    rows_s, cols_s = seam_indices(oh, ROW_SEAMS), seam_indices(ow, COL_SEAMS)
    strip_rows = set(seam_indices(oh, [4 * t for t in STRIP_TILES] if persistent else [16]))
    key = set()
    for r in rows_b:
        key.update(r * ow + c for c in range(ow))
    for c in cols_b:
        key.update(r * ow + c for r in range(oh))
    for r in rows_s:
        if r in strip_rows or len(cols_s) <= cross:
            cs = cols_s
        else:
            cs = [cols_s[i] for i in rng.choice(len(cols_s), size=cross, replace=False)]
        key.update(r * ow + c for c in cs)
    if fill and oh * ow:
        key.update(int(v) for v in rng.integers(0, oh * ow, size=fill))
    k = np.array(sorted(key), dtype=np.int64)
    return k // ow, k % ow


def wino3_strip(n, cin, cout, h, w, rgb=False, batch_invariant=False):
    """A RE-STATEMENT in Python of how csrc/wino3.hip's launch code chooses the persistent form's strip: (direction, tiles) or None for the
    one-shot kernel.  Computed, not observed -- the conv profile reports the kernel name and ksplit only -- so it labels reports (the census
    column, a failure's position) and states the strip-walk test's premise; if the rule moves in the .hip file this must be moved with it.
    What is gated does not depend on it: every persistent launch is sampled at the strip ends of 4, 8, 16 AND 32 tiles."""
    if cin != 32 or w % 32 or h % 4 or (rgb and cout != 32):
        return None
    tiles_x, tiles_y, co_tiles = w // 32, h // 4, -(-cout // 32)
    strip_len = min(tiles_x, 32)
    vlen = min(tiles_y, 32)
    while vlen > 4 and vlen % 2 == 0 and tiles_y % vlen == 0 and n * tiles_x * (tiles_y // vlen) * co_tiles < 2048:
        vlen //= 2
    vert = tiles_y % vlen == 0
    pcount = n * tiles_x * (tiles_y // vlen) * co_tiles if vert else n * (tiles_x // strip_len) * tiles_y * co_tiles
    if tiles_x % strip_len or (pcount < 2048 and not batch_invariant):
        return None
    return ("vertical", vlen) if vert else ("horizontal", strip_len)


# ----------------------------------------------------------------------------------------------------------------- evaluator
class Spec:
    """One launch in plain terms (tensors on any device, float32 as the kernel sees them).
    kind "corr":  y[n,co,oy,ox] = sum_t sum_ci w[t,ci,co] x[n,ci,oy*stride+dy_t,ox*stride+dx_t]      (0 outside x)
    kind "tconv": t[n,co,2i+kh,2j+kw] += w[kh*3+kw,ci,co] x[n,ci,i,j]                                 taps = the (kh, kw)
    w: [taps, cin, cout], or [n, taps, cin, cout] for per-sample weights.  in_scale [n, cin]; out_scale [n, cout] or [cout].
    A (the gate's denominator) = sum |w| |x| over the products; with bias_in_sum also + |bias| (see __init__).
    Epilogue (include/mgf.h): y = act(acc * out_scale + noise[n % noise_n] * strength + bias) * gain + residual (+ up2([1,3,3,1], low));
    act relu_post: y = relu((acc + bias) * gain + residual).  rgb = (rgb_w [n,c,cout], rgb_b | None): out[n,c] = rgb_w . y + rgb_b.
    residual is indexed like the output buffer: channel co of the launch is channel choff + co of it."""

    def __init__(self, kind, x, w, taps, oh, ow, stride=1, in_scale=None, out_scale=None, bias=None, noise=None, strength=None, noise_n=1,
                 act="linear", alpha=0.2, gain=1.0, residual=None, choff=0, residual_low=None, rgb=None, winograd=False, bias_in_sum=False,
                 mask=None):
        self.kind, self.x, self.w, self.taps, self.oh, self.ow, self.stride = kind, x, w, [tuple(t) for t in taps], oh, ow, stride
        self.in_scale, self.out_scale, self.bias, self.noise, self.strength, self.noise_n = in_scale, out_scale, bias, noise, strength, noise_n
        self.act, self.alpha, self.gain, self.residual, self.choff, self.residual_low, self.rgb = act, alpha, gain, residual, choff, residual_low, rgb
        self.winograd = winograd
        # bias_in_sum: the kernel's accumulator STARTS at the bias (conv3x3s2_few_inputs, csrc/narrow_conv.hip), so every rounding of its running sum is
        # relative to |bias + partial sum|: |bias| then belongs to the denominator A like any other addend of that sum.
        # mask = (a [n, cout, oh, ow], ring, slope): the MDF body adjoint's epilogue, y = acc * (a > 0 ? 1 : slope) on ring `ring`, exactly 0 outside
        self.bias_in_sum, self.mask = bias_in_sum, mask
        self.n, self.cin = x.shape[0], x.shape[1]
        self.cout = w.shape[-1]
        self.out_channels = rgb[0].shape[1] if rgb is not None else self.cout

    def copy(self, **kw):
        s = Spec.__new__(Spec)
        s.__dict__.update(self.__dict__)
        s.__dict__.update(kw)
        return s

    @property
    def products(self):
        return len(self.taps) * self.cin


def _up2_low(low, oy, ox, dt):
    """upfirdn2d(low, [1,3,3,1] x [1,3,3,1] / 64, up=2, padding [2,1,2,1], gain 4) at (oy, ox): per axis out[2i] = (low[i-1] + 3 low[i]) / 4,
    out[2i+1] = (3 low[i] + low[i+1]) / 4, zero outside.  low: [C, h2, w2] -> [C, P]."""
    h2, w2 = low.shape[-2:]

    def axis(o, size):
        i = torch.div(o, 2, rounding_mode="floor")
        odd = (o % 2) == 1
        j = torch.where(odd, i + 1, i - 1)                         # the neighbour with weight 1/4; i itself has 3/4
        ok = (j >= 0) & (j < size)
        return i, j.clamp(0, size - 1), ok
    iy, jy, oky = axis(oy, h2)
    ix, jx, okx = axis(ox, w2)
    lw = low.to(dt)
    z = lambda m: m.to(dt)
    return (9 * lw[:, iy, ix] + 3 * lw[:, jy, ix] * z(oky) + 3 * lw[:, iy, jx] * z(okx) + lw[:, jy, jx] * z(oky & okx)) / 16


def evaluate(spec, n_sel, c_sel, oy, ox, dtype=torch.float64, chunk=8192):
    """-> (val, A): [len(n_sel), len(c_sel), P] each, `val` the launch's result at out[n, choff + c, oy, ox] for the product of the three
    selections, computed in `dtype`; A = sum |w| |x| |in_scale| |out_scale| * gain over the same products (through |rgb_w| for a fused
    projection).  c_sel indexes the launch's OUTPUT channels (the rgb channels when a projection is fused)."""
    dev = spec.x.device
    oy = torch.as_tensor(oy, dtype=torch.int64, device=dev)
    ox = torch.as_tensor(ox, dtype=torch.int64, device=dev)
    c_sel = list(c_sel)
    conv_c = list(range(spec.cout)) if spec.rgb is not None else c_sel          # a projection needs every conv channel at the position
    ci = torch.as_tensor(conv_c, dtype=torch.int64, device=dev)
    h, w = spec.x.shape[2:]
    vals, As = [], []
    for n in n_sel:
        xn = spec.x[n].to(dtype)
        if spec.in_scale is not None:
            xn = xn * spec.in_scale[n].to(dtype)[:, None, None]
        wn = (spec.w[n] if spec.w.ndim == 4 else spec.w).to(dtype)[:, :, ci]                   # [taps, cin, C]
        wk = wn.reshape(-1, wn.shape[-1])
        outs_v, outs_a = [], []
        for p0 in range(0, oy.numel(), chunk):
            py, px = oy[p0:p0 + chunk], ox[p0:p0 + chunk]
            cols = []
            for (a, b) in spec.taps:
                if spec.kind == "corr":
                    iy, ix = py * spec.stride + a, px * spec.stride + b
                    ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
                else:
                    ty, tx = py - a, px - b
                    iy, ix = torch.div(ty, 2, rounding_mode="floor"), torch.div(tx, 2, rounding_mode="floor")
                    ok = (ty % 2 == 0) & (tx % 2 == 0) & (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
                cols.append(xn[:, iy.clamp(0, h - 1), ix.clamp(0, w - 1)] * ok.to(dtype))      # [cin, P]
            g = torch.stack(cols).reshape(-1, py.numel())                                       # [taps * cin, P]
            v = torch.matmul(wk.t(), g)                                                         # [C, P]
            a_ = torch.matmul(wk.abs().t(), g.abs())
            if spec.out_scale is not None:
                d = (spec.out_scale[n] if spec.out_scale.ndim == 2 else spec.out_scale).to(dtype)[ci][:, None]
                if spec.act == "relu_post":
                    raise Unexpressible("relu_post with an output scale")
                v, a_ = v * d, a_ * d.abs()
            res = None
            if spec.residual is not None:
                res = spec.residual[n][spec.choff + ci][:, py, px].to(dtype)
            if spec.act == "relu_post":
                if spec.noise is not None:
                    raise Unexpressible("relu_post with noise")
                if spec.bias is not None:
                    v = v + spec.bias.to(dtype)[ci][:, None]
                v = v * spec.gain
                if res is not None:
                    v = v + res
                v = torch.relu(v)
            else:
                if spec.noise is not None:
                    nz = spec.noise[n % spec.noise_n][py, px].to(dtype)
                    v = v + (nz * spec.strength.to(dtype).reshape(()) if spec.strength is not None else nz)[None]
                if spec.bias is not None:
                    v = v + spec.bias.to(dtype)[ci][:, None]
                if spec.act == "relu":
                    v = torch.relu(v)
                elif spec.act == "lrelu":
                    v = torch.where(v >= 0, v, v * spec.alpha)
                elif spec.act != "linear":
                    raise Unexpressible(f"activation {spec.act!r}")
                v = v * spec.gain
                if res is not None:
                    v = v + res
                if spec.residual_low is not None:
                    v = v + _up2_low(spec.residual_low[n][ci], py, px, dtype)
            if spec.bias_in_sum and spec.bias is not None:
                a_ = a_ + spec.bias.to(dtype)[ci].abs()[:, None]
            a_ = a_ * abs(spec.gain)
            if spec.mask is not None:
                am, ring, slope = spec.mask
                inside = ((py >= ring) & (py < spec.oh - ring) & (px >= ring) & (px < spec.ow - ring)).to(dtype)[None]
                f = torch.where(am[n][ci][:, py, px] > 0, torch.ones((), dtype=dtype, device=dev), torch.full((), slope, dtype=dtype, device=dev)) * inside
                v, a_ = v * f, a_ * f
            if spec.rgb is not None:
                rw = spec.rgb[0][n].to(dtype)                                                   # [c, cout]
                v, a_ = torch.matmul(rw, v), torch.matmul(rw.abs(), a_)
                if spec.rgb[1] is not None:
                    v = v + spec.rgb[1].to(dtype)[:, None]
                sel = torch.as_tensor(c_sel, dtype=torch.int64, device=dev)
                v, a_ = v[sel], a_[sel]
            outs_v.append(v)
            outs_a.append(a_)
        vals.append(torch.cat(outs_v, dim=1))
        As.append(torch.cat(outs_a, dim=1))
    return torch.stack(vals), torch.stack(As).to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------- comparator
def gate_constant(ref32, ref64, A, products, m):
    """c = max(m * r, sqrt(K) * 2^-24) with r = max |ref32 - ref64| / A over the sampled elements (A == 0: the element has no product)."""
    ok = A > 0
    r = float(((ref32.double() - ref64).abs()[ok] / A[ok]).max()) if bool(ok.any()) else 0.0
    return max(m * r, math.sqrt(products) * 2.0 ** -24), r


def compare(got, ref64, A, c, rel_bound=REL_BOUND):
    """-> dict(ok, worst ratio |got - ref64| / (c A) and its flat index, rel = max |got - ref64| / max |ref64|, nan)."""
    got = got.double()
    err = (got - ref64).abs()
    nan = bool(torch.isnan(got).any())
    bound = c * A
    # an element without products (A = 0: a border position no tap reaches) must equal its epilogue-only value to float32 rounding
    bound = torch.where(A > 0, bound, ref64.abs() * 2.0 ** -22)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst = int(ratio.argmax())
    rel = float(torch.nan_to_num(err, nan=float("inf")).max() / max(float(ref64.abs().max()), 1e-30))
    wr = float(ratio.reshape(-1)[worst])
    return {"ok": (not nan) and wr <= 1.0 and rel <= rel_bound, "worst": wr, "worst_index": worst, "rel": rel, "nan": nan}


def describe_position(n, co, oy, ox, strip=None):
    s = f"n={n} co={co} (tile {co // 32}, lane {co % 32}) oy={oy} (4-row tile {oy // 4}, row {oy % 4}; 32-row tile {oy // 32}, row {oy % 32}) " \
        f"ox={ox} (16-col tile {ox // 16}, col {ox % 16}; 32-col tile {ox // 32}, col {ox % 32})"
    if strip is not None:
        d, L = strip
        t = oy // 4 if d == "vertical" else ox // 32
        s += f"; {d} strip of {L} tiles: strip {t // L}, tile {t % L} of it"
    return s


# ------------------------------------------------------------------------------------------------------------------- replay
_DEVICE_DRAW = 1 << 24       # tensors from this many elements on are drawn on the device (a 32 x 32 x 1024^2 input takes the host seconds)


def _randn(gen, *shape):
    """Seeded normal draw: on the host below _DEVICE_DRAW elements, else on the device from a seed drawn from the host generator.  gen: (host generator, device)."""
    g, dev = gen
    if torch.device(dev).type != "cpu" and math.prod(shape) >= _DEVICE_DRAW:
        g2 = torch.Generator(device=dev).manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))
        return torch.randn(*shape, generator=g2, dtype=torch.float32, device=dev)
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def build_call(sig, device, seed):
    """-> (call, spec, info): call(cv) runs the recorded wrapper with the recorded options on fresh seeded data and returns
    (out buffer, choff, valid width), spec the plain description of that launch for `evaluate`; info: m, family, canary checks."""
    s = dict(sig)
    name = s["wrapper"]
    gen = (torch.Generator().manual_seed(seed), device)
    dv = lambda t: None if t is None else t.to(device).contiguous()
    if s["bf"]:
        raise Unexpressible("bf16x3 arithmetic is an engine mode of its own with its own bound (tests/test_hip_bf16x3.py)")
    n, cin, h, w = s["x"]
    x = dv(_randn(gen, n, cin, h, w))
    wsig = s["weight"]

    def scale(ssig, c, base, spread):
        if ssig is None:
            return None
        ndim, stride0, len0 = ssig
        if ndim == 1:
            return dv(base + spread * _randn(gen, c).clamp(-2.5, 2.5))
        if ndim != 2 or len0 != n:
            raise Unexpressible(f"scale of ndim {ndim} / leading length {len0} at batch {n}")
        t = dv(base + spread * _randn(gen, 1 if stride0 == 0 else n, c).clamp(-2.5, 2.5))
        return t.expand(n, c) if stride0 == 0 else t

    def epilogue(cout, oh, ow, out_shape):
        e = s["epilogue"]
        if e is None:
            return {}, None
        bias, noise, strength, noise_n, act, alpha, gain, residual = e
        if act not in ACT_NAMES:
            raise Unexpressible(f"activation id {act}")
        kw = {"act": ACT_NAMES[act], "alpha": alpha, "gain": gain, "noise_n": noise_n}
        if bias:
            kw["bias"] = dv(_randn(gen, cout))
        if noise:
            kw["noise"] = dv(_randn(gen, noise_n, oh, ow))
            if strength:
                kw["noise_strength"] = dv(torch.tensor([0.37]))
        elif strength:
            kw["noise_strength"] = dv(torch.tensor([0.37]))
        if residual:
            kw["residual"] = dv(_randn(gen, *out_shape))
        return kw, kw

    def spec_ep(kw):
        if not kw:
            return {}
        return {"bias": kw.get("bias"), "noise": kw.get("noise"), "strength": kw.get("noise_strength") if kw.get("noise") is not None else None,
                "noise_n": kw["noise_n"], "act": kw["act"], "alpha": kw["alpha"], "gain": kw["gain"], "residual": kw.get("residual")}

    def out_buffer(shape):
        return torch.full(shape, CANARY, dtype=torch.float32, device=device)

    from morphganformer_amd import _lib, conv as cvm
    info = {"m": M_DIRECT, "family": "tap-list / pointwise / narrow", "pitch_pad_from": None, "rel_bound": REL_BOUNDS[name],
            "written_everywhere": s["out"] is not None or name in ("tconv3x3s2_forward", "winograd2_rgb_forward") or s["rgb"] is not None}

    if name == "conv_forward":
        _, cout, wcin, kh, kw_, cout_pad = wsig
        ntaps = kh * kw_
        wt = _randn(gen, ntaps, cin, cout) / math.sqrt(ntaps * cin)
        wp = torch.zeros(ntaps, cin, cout_pad)
        wp[:, :, :cout] = wt
        pc = cvm.PackedConv(dv(wp), None, cout, cin, kh, kw_, cout_pad)
        py, px = s["pad"]
        kh_, kww = s["ksize"] if s["ksize"] is not None else (kh, kw_)
        stride = s["stride"]
        oh, ow = (h + 2 * py - kh_) // stride + 1, (w + 2 * px - kww) // stride + 1
        taps = list(s["taps"]) if s["taps"] is not None else [(a - py, b - px) for a in range(kh) for b in range(kw_)]
        ins, outs = scale(s["in_scale"], cin, 1.0, 0.3), scale(s["out_scale"], cout, 1.0, 0.2)
        if s["in_scale"] is not None and s["in_scale"][0] != 2:
            raise Unexpressible("conv_forward reads in_scale as [n, cin]")
        out_shape = s["out"] if (s["out"] is not None and s["rgb"] is None) else (n, cout, oh, ow)
        epkw, _ = epilogue(cout, oh, ow, out_shape)
        rgb = None
        if s["rgb"] is not None:
            rc, rb = s["rgb"]
            rgb = (dv(_randn(gen, n, rc, cout) / math.sqrt(cout)), dv(_randn(gen, rc)) if rb else None)
        spec = Spec("corr", x, dv(wt), taps, oh, ow, stride, ins, outs, choff=s["out_choff"], rgb=rgb, **spec_ep(epkw))

        def call(cv):
            ep = _lib.make_epilogue(**epkw) if epkw else None
            if rgb is not None:
                ro = out_buffer((n, rgb[0].shape[1], oh, ow))
                cv.conv_forward(x, pc, stride=stride, pad=(py, px), in_scale=ins, out_scale=outs, epilogue=ep, rgb=(rgb[0], rgb[1], ro),
                                taps=list(s["taps"]) if s["taps"] is not None else None, ksize=s["ksize"])
                return ro, 0, ow
            out = out_buffer(out_shape) if s["out"] is not None else None
            got = cv.conv_forward(x, pc, stride=stride, pad=(py, px), in_scale=ins, out_scale=outs, epilogue=ep, out=out, out_choff=s["out_choff"],
                                  taps=list(s["taps"]) if s["taps"] is not None else None, ksize=s["ksize"])
            return got, s["out_choff"], ow
        return call, spec, info

    if name in ("winograd_forward", "winograd2_forward", "winograd2_rgb_forward"):
        info.update(m=M_WINOGRAD, family="Winograd F(2x2,3x3)")
        if len(wsig) == 4:                                           # ("tensor", 16, cin, cout): form 1
            cout, form1 = wsig[3], True
        else:                                                        # ("tensor", 16, cin / 4, cout, 4)
            cout, form1 = wsig[3], False
        wt = _randn(gen, cout, cin, 3, 3) / (3 * math.sqrt(cin))
        taps = [(a - 1, b - 1) for a in range(3) for b in range(3)]
        wtaps = dv(wt.permute(2, 3, 1, 0).reshape(9, cin, cout))
        u = cvm.winograd_weights(dv(wt)) if form1 else cvm.winograd2_weights(dv(wt))
        ins, outs = scale(s["in_scale"], cin, 1.0, 0.3), scale(s["out_scale"], cout, 1.0, 0.2)
        if name == "winograd2_rgb_forward":
            rc, rb = s["rgb"]
            rgb = (dv(_randn(gen, n, rc, cout) / math.sqrt(cout)), dv(_randn(gen, rc)) if rb else None)
            spec = Spec("corr", x, wtaps, taps, h, w, 1, ins, outs, rgb=rgb, winograd=True)

            def call(cv):
                ro = out_buffer((n, rc, h, w))
                cv.winograd2_rgb_forward(x, u, rgb[0], rgb[1], ro, in_scale=ins, out_scale=outs)
                return ro, 0, w
            return call, spec, info
        out_shape = s["out"] if s["out"] is not None else (n, cout, h, w)
        epkw, _ = epilogue(cout, h, w, out_shape)
        low = dv(_randn(gen, n, cout, h // 2, w // 2)) if s["residual_low"] else None
        spec = Spec("corr", x, wtaps, taps, h, w, 1, ins, outs, choff=s["out_choff"], residual_low=low, winograd=True, **spec_ep(epkw))

        def call(cv):
            ep = _lib.make_epilogue(**epkw) if epkw else None
            out = out_buffer(out_shape) if s["out"] is not None else None
            if name == "winograd_forward":
                got = cv.winograd_forward(x, u, in_scale=ins, out_scale=outs, epilogue=ep, out=out, residual_low=low)
            else:
                got = cv.winograd2_forward(x, u, in_scale=ins, out_scale=outs, epilogue=ep, out=out, out_choff=s["out_choff"], residual_low=low)
            return got, s["out_choff"], w
        return call, spec, info

    if name == "tconv3x3s2_forward":
        _, cout, wcin, kh, kw_, cout_pad = wsig
        wt = _randn(gen, cout, cin, 3, 3) / math.sqrt(9 * cin)
        wtaps = wt.permute(2, 3, 1, 0).reshape(9, cin, cout)
        wp = torch.zeros(9, cin, cout_pad)
        wp[:, :, :cout] = wtaps
        pc = cvm.PackedConv(dv(wp), None, cout, cin, 3, 3, cout_pad)
        wtw = cvm.tconv_winograd_weights(dv(wt)) if s["wt"] else None
        ins, outs = scale(s["in_scale"], cin, 1.0, 0.2), scale(s["out_scale"], cout, 1.0, 0.2)
        oh, ow = 2 * h + 1, 2 * w + 1
        spec = Spec("tconv", x, dv(wtaps), [(a, b) for a in range(3) for b in range(3)], oh, ow, 1, ins, outs)
        pitch = s["out"][3] if s["out"] is not None else cvm.tconv_pitch(w)
        info["pitch_pad_from"] = ow
        # (a launch that turns out to be wino_tconv_kernel is gated at the Winograd constant: _gate reads it off the replayed launch's name)

        def call(cv):
            out = out_buffer((n, cout, oh, pitch))                     # the wrapper returns a view of it: keep the padded buffer for the canary
            cv.tconv3x3s2_forward(x, pc, in_scale=ins, out_scale=outs, out=out, wt=wtw)
            return out, 0, ow
        return call, spec, info

    if name == "conv3x3_few_outputs":
        _, wn, cout, wcin, _, _ = wsig
        wt = _randn(gen, n, cout, cin, 3, 3) / (3 * math.sqrt(cin))
        bias = dv(_randn(gen, cout)) if s["bias"] else None
        wd = dv(wt)
        spec = Spec("corr", x, dv(wt.permute(0, 3, 4, 2, 1).reshape(n, 9, cin, cout)), [(a - 1, b - 1) for a in range(3) for b in range(3)], h, w, 1,
                    bias=bias)

        def call(cv):
            out = out_buffer(s["out"]) if s["out"] is not None else None
            return cv.conv3x3_few_outputs(x, wd, bias=bias, out=out), 0, w
        return call, spec, info

    if name == "conv3x3s2_few_inputs":
        _, cout, wcin, _, _ = wsig
        wt = _randn(gen, cout, cin, 3, 3) / (3 * math.sqrt(cin))
        bias = dv(_randn(gen, cout)) if s["bias"] else None
        wd = dv(wt)
        oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        spec = Spec("corr", x, dv(wt.permute(2, 3, 1, 0).reshape(9, cin, cout)), [(a, b) for a in range(3) for b in range(3)], oh, ow, 2, bias=bias,
                    act="relu" if s["relu"] else "linear", bias_in_sum=True)

        def call(cv):
            out = out_buffer(s["out"]) if s["out"] is not None else None
            return cv.conv3x3s2_few_inputs(x, wd, bias=bias, relu=s["relu"], out=out), 0, ow
        return call, spec, info
    raise Unexpressible(f"wrapper {name}")


def stable_seed(sig):
    """The data seed of a record: a hash of its own signature, so that no other record's presence or order can change it."""
    return zlib.crc32(repr(sig).encode()) & 0x7FFFFFFF


def replay(cv, sig, device="cuda", seed=None, fill=2048):
    """Replay one record and gate it.  -> dict(ok, launches, worst, rel, r, c, headroom = max |got - ref64| / (r A), where, problems)."""
    seed = stable_seed(sig) if seed is None else seed
    call, spec, info = build_call(sig, device, seed)
    return _gate(cv, call, spec, info, device, seed, fill)


def _gate(cv, call, spec, info, device, seed, fill, min_ring=0):
    cv.profile_begin()
    try:
        got, choff, valid_w = call(cv)
    finally:
        launches = tuple((r[0], r[3]) for r in cv.profile_end(64))
    torch.cuda.synchronize()
    if any(k == "wino_tconv_kernel" for k, _ in launches):
        # Winograd on the 2h x 2w quads, direct on row 2h / column 2w: one constant for the whole workspace, the wider one
        info.update(m=M_WINOGRAD, family="polyphase Winograd transposed conv")
    n, cout_o = spec.n, spec.out_channels
    rgbf = spec.rgb is not None
    strip = wino3_strip(n, spec.cin, spec.cout, spec.oh, spec.ow, rgbf, info.get("batch_invariant", False)) if spec.winograd else None
    persistent = any("wino3p" in k for k, _ in launches)
    n_sel, c_sel = select_samples(n), (list(range(cout_o)) if rgbf else select_channels(cout_o, seed))
    oy, ox = select_positions(spec.oh, spec.ow, persistent=persistent, fill=fill, seed=seed)
    if min_ring:                                                   # (the MDF body's outermost ring is not part of its contract)
        keep = (oy >= min_ring) & (oy < spec.oh - min_ring) & (ox >= min_ring) & (ox < spec.ow - min_ring)
        oy, ox = oy[keep], ox[keep]
    ref64, A = evaluate(spec, n_sel, c_sel, oy, ox, torch.float64)
    ref32, _ = evaluate(spec, n_sel, c_sel, oy, ox, torch.float32)
    c, r = gate_constant(ref32, ref64, A, spec.products, info["m"])
    ty, tx = torch.as_tensor(oy, device=device), torch.as_tensor(ox, device=device)
    ni = torch.as_tensor(n_sel, device=device)
    cix = torch.as_tensor(c_sel, device=device) + choff
    g = got[ni[:, None, None], cix[None, :, None], ty[None, None, :], tx[None, None, :]]
    res = compare(g, ref64, A, c, info["rel_bound"])
    problems = []
    if min_ring == 0 and bool(torch.isnan(got).any()):
        problems.append("NaN in the output buffer")
    if got.shape[1] > choff + cout_o or choff:                     # a channel slice of a wider buffer: the rest keeps the canary, bit for bit
        mask = torch.ones(got.shape[1], dtype=torch.bool, device=device)
        mask[choff:choff + cout_o] = False
        if not bool((got[:, mask] == CANARY).all()):
            problems.append("a float outside the written channel slice changed")
    if info["pitch_pad_from"] is not None and got.shape[3] > info["pitch_pad_from"]:
        if not bool((got[:, :, :, info["pitch_pad_from"]:] == CANARY).all()):
            problems.append("a pad float of the transposed conv's pitch changed")
    if info["written_everywhere"]:
        if bool((got[:, choff:choff + cout_o, :, :valid_w] == CANARY).any()):
            problems.append("an element of the written slice still holds the canary (not written)")
    i = res["worst_index"]
    P = len(oy)
    wn, wc, wp_ = i // (len(c_sel) * P), (i // P) % len(c_sel), i % P
    res.update(launches=launches, r=r, c=c, m=info["m"], family=info["family"], strip=strip, rel_bound=info["rel_bound"],
               headroom=res["worst"] * c / r if r > 0 else float("nan"), elements=len(n_sel) * len(c_sel) * P,
               where=describe_position(n_sel[wn], c_sel[wc], int(oy[wp_]), int(ox[wp_]), strip), problems=problems)
    res["ok"] = res["ok"] and not problems
    return res


# MDF: the discriminators' body layers reach the form-3 launch through mgf_mdf_body_f32 / mgf_mdf_body_backward_f32 (the batch-invariant
# dispatch: the kernel and its strip follow (cin, h, w) alone), not through a wrapper of conv.py, so there is no call to record.  The launches the
# objective makes at 1024^2 with the eight-discriminator fixture (N = 32 / 64; 128 is the ninth discriminator's width) are replayed directly:
# forward at 32 candidates and at one, the masked adjoint at one (gradient mode).
MDF_CASES = [(kind, n, c) for c in (32, 64, 128) for kind, n in (("mdf_body", 32), ("mdf_body", 1), ("mdf_body_backward", 1))]
MDF_SLOPE = 0.2


def replay_mdf(cv, kind, n, c, h=1024, w=1024, device="cuda", fill=2048):
    from morphganformer_amd import _lib
    from morphganformer_amd.mdf import adjoint_weights
    L = _lib.lib()
    seed = stable_seed((kind, n, c, h, w))
    gen = (torch.Generator().manual_seed(seed), device)
    x = _randn(gen, n, c, h, w).to(device)
    wt = _randn(gen, c, c, 3, 3) * math.sqrt(2.0 / (9 * c))
    taps = [(a - 1, b - 1) for a in range(3) for b in range(3)]
    info = {"m": M_WINOGRAD, "family": "Winograd F(2x2,3x3)", "pitch_pad_from": None, "rel_bound": REL_BOUNDS[kind], "written_everywhere": False,
            "batch_invariant": True}
    if kind == "mdf_body":
        bias = (0.1 * _randn(gen, c)).to(device)
        u = cv.winograd2_weights(wt.to(device))
        spec = Spec("corr", x, wt.permute(2, 3, 1, 0).reshape(9, c, c).to(device), taps, h, w, bias=bias, act="lrelu", alpha=MDF_SLOPE, winograd=True)

        def call(cv_):
            y = torch.full((n, c, h, w), CANARY, dtype=torch.float32, device=device)
            _lib.check(L.mgf_mdf_body_f32(y.data_ptr(), x.data_ptr(), u.data_ptr(), bias.data_ptr(), n, c, h, w, MDF_SLOPE, _lib.stream_ptr()), kind)
            return y, 0, w
        return _gate(cv, call, spec, info, device, seed, fill, min_ring=1)       # the valid 3x3 of the frame: rows / columns 1 .. h-2 / w-2
    ring = {32: 1, 64: 2, 128: 3}[c]
    x[:, :, :ring + 1] = 0; x[:, :, h - ring - 1:] = 0; x[:, :, :, :ring + 1] = 0; x[:, :, :, w - ring - 1:] = 0       # the incoming gradient lives on ring + 1
    a = _randn(gen, n, c, h, w).to(device)
    wadj = torch.as_tensor(adjoint_weights(wt.numpy()), dtype=torch.float32)
    u = cv.winograd2_weights(wadj.to(device))
    spec = Spec("corr", x, wadj.permute(2, 3, 1, 0).reshape(9, c, c).contiguous().to(device), taps, h, w, winograd=True, mask=(a, ring, MDF_SLOPE))
    info["written_everywhere"] = True

    def call(cv_):
        d = torch.full((n, c, h, w), CANARY, dtype=torch.float32, device=device)
        _lib.check(L.mgf_mdf_body_backward_f32(d.data_ptr(), x.data_ptr(), u.data_ptr(), a.data_ptr(), n, c, h, w, ring, MDF_SLOPE, _lib.stream_ptr()), kind)
        return d, 0, w
    return _gate(cv, call, spec, info, device, seed, fill)


def format_sig(sig):
    s = dict(sig)
    keep = {k: v for k, v in s.items() if v not in (None, False) and not (k in ("stride",) and v == 1) and not (k == "out_choff" and v == 0)}
    return " ".join(f"{k}={v}" for k, v in keep.items())


# ---------------------------------------------------------------------------------------------------------------- workloads
# The production workloads, each built as bench.py / tests/test_hip_fullsize.py build them (synth_weights.FULL1024, seeded random backbones),
# eager (use_graph=False: only the calls matter).  MDF makes no wrapper call: its launches are replayed directly (replay_mdf above).
_CACHE = {}


def _generator(max_batch=1):
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import FULL1024 as cfg, make_state_dict, synthetic_latents
    if "sd" not in _CACHE:
        _CACHE["sd"] = make_state_dict(cfg, seed=0)
    G = Generator(_CACHE["sd"], cfg, "cuda", max_batch=max_batch)
    if "target" not in _CACHE:
        _CACHE["target"] = G(torch.from_numpy(synthetic_latents(cfg, 1, 1000)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone()
    return cfg, G, _CACHE["target"]


def _candidates(n, seed=3):
    """n images near the target, in [-1, 1] (what the loss networks see in the loop)."""
    _, _, target = _generator()
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (target + 0.2 * torch.randn(n, *target.shape[1:], device="cuda", generator=g)).clamp(-1, 1).contiguous()


def wl_literal32():
    """The headline: literal loop, 1024^2, 32 candidates per forward, LPIPS(squeeze) + MSE + Wing, composed ToRGB."""
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine, latent_stats, synthetic_landmarks
    cfg, G, target = _generator()
    G.fuse_torgb = True
    gen = torch.Generator(device="cuda").manual_seed(0)
    mean, std = latent_stats(G, 10000, "cuda", gen)
    P = PerceptualLoss(model="net-lin", net="squeeze", use_gpu=True, device="cuda", allow_random_backbone=True)
    lm_t, lm_s = synthetic_landmarks(64, cfg.img_resolution, seed=7)
    eng = ProjectionEngine(G, target, mean, std, ProjectionArgs(step=64), percept=P, use_mse=True, lm_target=lm_t, lm_steps=lm_s,
                           noise_mode="random", seed=100, use_graph=False, batch=32, gamma=1e-6)
    eng.run(64)
    torch.cuda.synchronize()


def wl_literal32_fused_torgb():
    """The generator forward of the loop with the composed conv_last + ToRGB map switched off (MGF_TORGB_COMPOSE=0 semantics: the full
    conv_last with the projection fused into its epilogue)."""
    from morphganformer_amd.synth_weights import synthetic_latents
    cfg, G, _ = _generator(max_batch=32)
    G.fuse_torgb, G.torgb_compose = True, False
    G(torch.from_numpy(synthetic_latents(cfg, 32, 5)).cuda(), None, noise_mode="random")
    torch.cuda.synchronize()


def wl_generator_b1():
    from morphganformer_amd.synth_weights import synthetic_latents
    cfg, G, _ = _generator()
    G(torch.from_numpy(synthetic_latents(cfg, 1, 6)).cuda(), None, noise_mode="const")
    torch.cuda.synchronize()


def _gradient(B):
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, latent_stats, synthetic_landmarks
    from morphganformer_amd.synth_weights import synthetic_latents
    cfg, G, target = _generator(max_batch=B)
    gen = torch.Generator(device="cuda").manual_seed(0)
    mean, _ = latent_stats(G, 10000, "cuda", gen)
    P = PerceptualLoss(model="net-lin", net="squeeze", use_gpu=True, device="cuda", allow_random_backbone=True)
    if B == 1:
        lm_t, lm_s = synthetic_landmarks(8, cfg.img_resolution, seed=7)
        tg = target
    else:
        zt = torch.from_numpy(synthetic_latents(cfg, B, seed=2000)).cuda()
        tg = torch.cat([G(zt[j:j + 1], None, noise_mode="const")[0].clamp(-1, 1) for j in range(B)]).contiguous()
        lm = [synthetic_landmarks(8, cfg.img_resolution, seed=50 + j) for j in range(B)]
        lm_t, lm_s = np.stack([l[0] for l in lm]), np.stack([l[1] for l in lm])
    ge = GradientProjectionEngine(G, tg, mean, 1.0, ProjectionArgs(step=8), percept=P, use_mse=True, lm_target=lm_t, lm_steps=lm_s,
                                  noise_mode="random", seed=5, use_graph=False)
    ge.run(2)
    torch.cuda.synchronize()


def wl_gradient1():
    """Gradient mode at one target: forward + LPIPS forward / backward + generator backward."""
    _gradient(1)


def wl_gradient8():
    """Gradient mode, 8 targets in lockstep."""
    _gradient(8)


def _lpips(net):
    from morphganformer_amd.lpips import PerceptualLoss
    _, _, target = _generator()
    P = PerceptualLoss(model="net-lin", net=net, use_gpu=True, device="cuda", allow_random_backbone=True)
    P.set_target(target)
    imgs = _candidates(32)
    P.distance_into(torch.zeros(32, device="cuda"), imgs)
    one = imgs[:1].contiguous()
    P.distance_into(torch.zeros(1, device="cuda"), one, keep_taps=True)
    P.grad_into(torch.zeros_like(one), scale=1.0, accumulate=False)
    torch.cuda.synchronize()


def wl_lpips_squeeze():
    _lpips("squeeze")


def wl_lpips_alex():
    _lpips("alex")


def wl_lpips_vgg():
    _lpips("vgg")


def wl_facenet():
    """FaceNet (InceptionResnetV1) on the un-resized 1024^2 image: forward at 16 candidates, forward + backward at one."""
    from morphganformer_amd.facenet import random_state
    from morphganformer_amd.iresnet import BiometricLoss
    _, _, target = _generator()
    sd = random_state(0)
    imgs = _candidates(16)
    bio = BiometricLoss("facenet", state=sd, n=16)
    bio.set_target(target)
    bio.distance_into(torch.zeros(16, device="cuda"), imgs)
    one = BiometricLoss("facenet", state=sd, n=1)
    one.embedder.keep_activations = True
    one.set_target(target)
    img1 = imgs[:1].contiguous()
    one.distance_into(torch.zeros(1, device="cuda"), img1)
    one.grad_into(torch.zeros_like(img1), scale=1.0, accumulate=False)
    torch.cuda.synchronize()


def wl_iresnet50():
    from morphganformer_amd.iresnet import BiometricLoss, IResNetEmbedder
    _, _, target = _generator()
    bio = BiometricLoss(IResNetEmbedder(None, depth=50, n=32, device="cuda", seed=0))
    bio.set_target(target)
    bio.distance_into(torch.zeros(32, device="cuda"), _candidates(32))
    torch.cuda.synchronize()


WORKLOADS = {"literal32": wl_literal32, "literal32_fused_torgb": wl_literal32_fused_torgb, "generator_b1": wl_generator_b1,
             "gradient1": wl_gradient1, "gradient8": wl_gradient8, "lpips_squeeze": wl_lpips_squeeze, "lpips_alex": wl_lpips_alex,
             "lpips_vgg": wl_lpips_vgg, "facenet": wl_facenet, "iresnet50": wl_iresnet50}


def record_workload(cv, name):
    _generator()                     # the cached state dict and target image are built OUTSIDE the bracket: a workload's records are its own
    with Recorder(cv) as rec:
        WORKLOADS[name]()
    return rec


def strip_walk_records():
    """Persistent form-3 launches at cin = 32, 1024 x 1024, n = 1, 2, 4, 8 (vertical strips of 4 / 8 / 16 / 32 tiles by the launch code's own
    rule): plain / full-resolution residual / half-resolution residual / ToRGB.  -> [(n, case, signature)]."""
    out = []
    ep = (True, True, True, None, 3, 0.2, round(math.sqrt(2.0), 7), False)
    for n in (1, 2, 4, 8):
        base = {"wrapper": "winograd_forward", "x": (n, 32, 1024, 1024), "weight": ("tensor", 16, 8, 32, 4), "stride": 1, "pad": None, "taps": None,
                "ksize": None, "in_scale": (2, 32, n), "out_scale": (2, 32, n), "out": None, "out_choff": 0, "residual_low": False, "rgb": None,
                "bf": False, "wt": False, "bias": False, "relu": False}
        e = ep[:3] + (n,) + ep[4:]
        cases = {"plain": dict(base, epilogue=e), "residual": dict(base, epilogue=e[:7] + (True,)),
                 "half-resolution residual": dict(base, epilogue=e, residual_low=True),
                 "ToRGB": dict(base, wrapper="winograd2_rgb_forward", epilogue=None, rgb=(3, True), out=(n, 3, 1024, 1024))}
        out += [(n, k, tuple(sorted(v.items()))) for k, v in cases.items()]
    return out


# conv_taps_kernel<WM, WN, MODE, ...> workgroup tiles.  The workloads reach all six (profiles/conv_launch_census.txt) -- 1 x 3 and 1 x 4 only
# in gradient mode and the loss networks, 1 x 1 and 1 x 2 only as transposed convs (MODE 1) -- so each of these four gets one direct replay
# case at the smallest shape that selects it by csrc/conv_taps.hip's rule (<= 32 output channels; 1 x 3 / 1 x 4 from 512 * 64 positions).
def direct_tile_records():
    base = {"wrapper": "conv_forward", "stride": 1, "pad": (1, 1), "taps": None, "ksize": None, "in_scale": None, "out_scale": None, "epilogue": None,
            "out": None, "out_choff": 0, "residual_low": False, "rgb": None, "bf": False, "wt": False, "bias": False, "relu": False}
    return {k: tuple(sorted(dict(base, **v).items())) for k, v in DIRECT_TILE_CASES.items()}


DIRECT_TILE_CASES = {
    # 3x3, <= 32 output channels, a map of 512 * 64 positions: the 1 x 3 tile (12-row tiles)
    "conv_taps_kernel<1, 3,": {"x": (1, 8, 128, 256), "weight": ("packed", 20, 8, 3, 3, 32)},
    # 1x1 with an output scale (so that it is not the register-operand GEMM of csrc/pointwise.hip), same map: the 1 x 4 tile (16-row tiles)
    "conv_taps_kernel<1, 4,": {"x": (2, 8, 128, 256), "weight": ("packed", 20, 8, 1, 1, 32), "pad": (0, 0), "out_scale": (2, 20, 2)},
    # <= 32 output channels on a smaller map: the 1 x 2 tile in its stride-1 mode (the workloads reach 1 x 2 as a transposed conv only)
    "conv_taps_kernel<1, 2, 0,": {"x": (2, 8, 40, 64), "weight": ("packed", 20, 8, 3, 3, 32)},
    # ... and on a map of at most 128 positions: the 1 x 1 tile in its stride-1 mode
    "conv_taps_kernel<1, 1, 0,": {"x": (2, 8, 8, 16), "weight": ("packed", 20, 8, 3, 3, 32)},
}
