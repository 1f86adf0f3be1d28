"""The replay gate of tests/conv_replay.py must be able to fail: on the CPU, with the float32 run of the evaluator standing in for a kernel's
output, every defect the gate exists for -- applied to the float64 reference -- is flagged at the constant c the gate forms from the
reference alone, and the unmutated pair passes.  Also the evaluator against torch's own float64 convolutions (CPU), the recorder's
de-duplication, and the seam / border selection as index arithmetic."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_replay as cr  # noqa: E402

LAYERS = [(32, 32, 64, "corr"), (512, 512, 16, "corr"), (128, 64, 32, "tconv")]        # (cin, cout, h[, -> transposed conv])
TAPS3 = [(a - 1, b - 1) for a in range(3) for b in range(3)]


def _layer(cin, cout, h, kind, n=2, seed=0, low=True):
    g = torch.Generator().manual_seed(seed + cin + h)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(n, cin, h, h)
    wt = r(cout, cin, 3, 3) / (3 * math.sqrt(cin))
    wtaps = wt.permute(2, 3, 1, 0).reshape(9, cin, cout).contiguous()
    s, d = 1 + 0.3 * r(n, cin).clamp(-2.5, 2.5), 1 + 0.2 * r(n, cout).clamp(-2.5, 2.5)
    if kind == "tconv":
        return cr.Spec("tconv", x, wtaps, [(a, b) for a in range(3) for b in range(3)], 2 * h + 1, 2 * h + 1, 1, s, d), wt
    spec = cr.Spec("corr", x, wtaps, TAPS3, h, h, 1, s, d, bias=r(cout), noise=r(n, h, h), strength=torch.tensor([0.37]), noise_n=n, act="lrelu",
                   alpha=0.2, gain=math.sqrt(2.0), residual_low=r(n, cout, h // 2, h // 2) if low else None)
    return spec, wt


def _sel(spec, seed=0):
    oy, ox = cr.select_positions(spec.oh, spec.ow, persistent=True, fill=512, seed=seed)
    return cr.select_samples(spec.n), cr.select_channels(spec.out_channels, seed), oy, ox


def _gate(spec, mutated, where=None, m=cr.M_DIRECT):
    """ref32 of `spec` (the stand-in for a kernel) against the float64 reference of `mutated`, taken only at the elements `where` selects
    (the unmutated reference elsewhere).  -> compare()'s result at the c formed from the UNMUTATED pair."""
    n_sel, c_sel, oy, ox = _sel(spec)
    ref64, A = cr.evaluate(spec, n_sel, c_sel, oy, ox, torch.float64)
    ref32, _ = cr.evaluate(spec, n_sel, c_sel, oy, ox, torch.float32)
    c, r = cr.gate_constant(ref32, ref64, A, spec.products, m)
    assert c >= math.sqrt(spec.products) * 2.0 ** -24 and r > 0
    bad = ref64
    if mutated is not None:
        mut, _ = (cr.evaluate(mutated, n_sel, c_sel, oy, ox, torch.float64) if isinstance(mutated, cr.Spec) else (mutated(ref64), None))
        if where is None:
            bad = mut
        else:
            mask = where(torch.as_tensor(n_sel)[:, None, None], torch.as_tensor(c_sel)[None, :, None], torch.as_tensor(oy)[None, None, :],
                         torch.as_tensor(ox)[None, None, :])
            assert bool(mask.any()), "the mutation touches no sampled element"
            bad = torch.where(mask.expand_as(ref64), mut, ref64)
    return cr.compare(ref32, bad, A, c), (n_sel, c_sel, oy, ox)


@pytest.mark.parametrize("cin,cout,h,kind", LAYERS)
@pytest.mark.parametrize("m", [cr.M_DIRECT, cr.M_WINOGRAD])
def test_unmutated_pair_passes(cin, cout, h, kind, m):
    spec, _ = _layer(cin, cout, h, kind)
    res, _ = _gate(spec, None, m=m)
    assert res["ok"] and res["worst"] <= 1.0 / m + 1e-12, res


def _zero_w(spec, taps=slice(None), ci=slice(None), co=slice(None)):
    w = spec.w.clone()
    w[taps, ci, co] = 0
    return spec.copy(w=w)


MUTATIONS = ["tap_last_column", "chunk4", "chunk8", "noise_shift", "out_scale_swap", "low_shift", "splitk_slice", "border_row_zero"]
# (the transposed conv has no epilogue -- no noise map, no half-resolution residual -- and only it has a row 2h)
CASES = [(l, mu) for l in LAYERS for mu in MUTATIONS
         if not (l[3] == "tconv" and mu in ("noise_shift", "low_shift")) and not (l[3] != "tconv" and mu == "border_row_zero")]


@pytest.mark.parametrize("layer,mutation", CASES, ids=[f"{l[0]}-{l[1]}-{l[2]}-{l[3]}-{mu}" for l, mu in CASES])
@pytest.mark.parametrize("m", [cr.M_DIRECT, cr.M_WINOGRAD])
def test_every_mutation_is_flagged(layer, m, mutation):
    """Each defect, at the size one wrong seam / slice / chunk has, is flagged at BOTH constants (m = 4 and the Winograd forms' m = 8): if one
    were not, m would be too large."""
    cin, cout, h, kind = layer
    spec, _ = _layer(cin, cout, h, kind)
    tconv = kind == "tconv"
    last = spec.ow - 1
    where = None
    if mutation == "tap_last_column":
        # one tap that reaches the last column (corr: the centre tap; tconv: kw = 2 is the only column tap there, take (0, 2)) dropped along it
        mut = _zero_w(spec, taps=(2 if tconv else 4))
        where = lambda n, c, oy, ox: ox == last
    elif mutation in ("chunk4", "chunk8"):
        k = 4 if mutation == "chunk4" else 8
        mut = _zero_w(spec, ci=slice(cin - k, cin), co=slice(0, 32))                # one chunk of input channels missing in the first 32-wide tile
    elif mutation == "noise_shift":
        mut = spec.copy(noise=torch.roll(spec.noise, 1, dims=2))
    elif mutation == "out_scale_swap":
        d = spec.out_scale.clone()
        d[0] = spec.out_scale[1]
        mut = spec.copy(out_scale=d)
    elif mutation == "low_shift":
        mut = spec.copy(residual_low=torch.roll(spec.residual_low, 1, dims=3))
    elif mutation == "splitk_slice":
        ksplit = max(2, cin // 64)                                                  # the last of ksplit K slices missing for ONE tile: rows < 4, channels < 32
        mut = _zero_w(spec, ci=slice(cin - cin // ksplit, cin), co=slice(0, 32))
        where = lambda n, c, oy, ox: (oy < 4) & (ox < 32) & (c < 32) & (n == 0)
    elif mutation == "border_row_zero":
        mut = lambda ref: torch.zeros_like(ref)
        where = lambda n, c, oy, ox: oy == spec.oh - 1
    res, _ = _gate(spec, mut, where, m=m)
    assert not res["ok"] and res["worst"] > 1.0, (mutation, res)


@pytest.mark.parametrize("stride,pad,k", [(1, 1, 3), (2, 0, 3), (1, 0, 1), (2, 1, 3)])
def test_evaluator_matches_torch_float64_convolution(stride, pad, k):
    """The evaluator is itself checked (CPU, float64): tap-list correlation with stride / pad, scales, the whole epilogue and the fused projection."""
    from oracle.ops_ref import bias_act_ref
    g = torch.Generator().manual_seed(k + stride)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n, cin, cout, h, w = 3, 12, 40, 21, 38
    x, wt, s, d = r(n, cin, h, w), r(cout, cin, k, k), 1 + 0.3 * r(n, cin), 1 + 0.2 * r(n, cout)
    conv = torch.nn.functional.conv2d(x * s[:, :, None, None], wt, stride=stride, padding=pad) * d[:, :, None, None]
    oh, ow = conv.shape[2:]
    noise, bias, resid = r(2, oh, ow), r(cout), r(n, cout + 8, oh, ow)
    ref = bias_act_ref(conv + 0.37 * noise[torch.arange(n) % 2][:, None], bias, act="lrelu", alpha=0.2, gain=1.3) + resid[:, 8:]
    taps = [(a - pad, b - pad) for a in range(k) for b in range(k)]
    spec = cr.Spec("corr", x, wt.permute(2, 3, 1, 0).reshape(k * k, cin, cout), taps, oh, ow, stride, s, d, bias=bias, noise=noise,
                   strength=torch.tensor([0.37], dtype=torch.float64), noise_n=2, act="lrelu", alpha=0.2, gain=1.3, residual=resid, choff=8)
    oy, ox = np.divmod(np.arange(oh * ow), ow)
    got, A = cr.evaluate(spec, range(n), range(cout), oy, ox)
    assert float((got.reshape(n, cout, oh, ow) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    absref = torch.nn.functional.conv2d((x * s[:, :, None, None]).abs(), wt.abs(), stride=stride, padding=pad) * d.abs()[:, :, None, None] * 1.3
    assert float((A.reshape(n, cout, oh, ow) - absref).abs().max()) <= 1e-12 * float(absref.abs().max())
    rw, rb = r(n, 3, cout), r(3)
    plain = cr.Spec("corr", x, spec.w, taps, oh, ow, stride, s, d, rgb=(rw, rb))
    got, _ = cr.evaluate(plain, range(n), range(3), oy, ox)
    want = torch.einsum("nkc,nchw->nkhw", rw, conv) + rb[None, :, None, None]
    assert float((got.reshape(n, 3, oh, ow) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    relu_post = cr.Spec("corr", x, spec.w, taps, oh, ow, stride, s, None, bias=bias, act="relu_post", gain=0.17, residual=resid, choff=8)
    got, _ = cr.evaluate(relu_post, range(n), range(cout), oy, ox)
    want = torch.relu((torch.nn.functional.conv2d(x * s[:, :, None, None], wt, stride=stride, padding=pad) + bias[None, :, None, None]) * 0.17 + resid[:, 8:])
    assert float((got.reshape(n, cout, oh, ow) - want).abs().max()) <= 1e-12


def test_evaluator_transposed_conv_per_sample_weights_and_half_resolution_residual():
    from oracle.ops_ref import setup_filter_ref, upfirdn2d_ref
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n, cin, cout, h, w = 2, 8, 36, 7, 10
    x, wt, s, d = r(n, cin, h, w), r(cout, cin, 3, 3), 1 + 0.2 * r(n, cin), 1 + 0.2 * r(cout)
    ref = torch.nn.functional.conv_transpose2d(x * s[:, :, None, None], wt.transpose(0, 1), stride=2) * d[None, :, None, None]
    oh, ow = ref.shape[2:]
    assert (oh, ow) == (2 * h + 1, 2 * w + 1)
    spec = cr.Spec("tconv", x, wt.permute(2, 3, 1, 0).reshape(9, cin, cout), [(a, b) for a in range(3) for b in range(3)], oh, ow, 1, s, d)
    oy, ox = np.divmod(np.arange(oh * ow), ow)
    got, A = cr.evaluate(spec, range(n), range(cout), oy, ox)
    assert float((got.reshape(n, cout, oh, ow) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool((A > 0).all())
    # per-sample weights (the composed conv_last + ToRGB map) and the half-resolution residual of the resnet skip branch
    h, w = 8, 12
    x, wn, low = r(n, cin, h, w), r(n, 3, cin, 3, 3), r(n, 3, h // 2, w // 2)
    want = torch.stack([torch.nn.functional.conv2d(x[i:i + 1], wn[i], padding=1)[0] for i in range(n)])
    skip = upfirdn2d_ref(low.float(), setup_filter_ref([1, 3, 3, 1]), up=2, padding=[2, 1, 2, 1], gain=4.0).double()
    spec = cr.Spec("corr", x, wn.permute(0, 3, 4, 2, 1).reshape(n, 9, cin, 3), TAPS3, h, w, residual_low=low.float().double())
    oy, ox = np.divmod(np.arange(h * w), w)
    got, _ = cr.evaluate(spec, range(n), range(3), oy, ox)
    assert float((got.reshape(n, 3, h, w) - (want + skip)).abs().max()) <= 1e-6 * float(want.abs().max())


def test_selection_covers_borders_seams_and_strip_ends():
    oh, ow = 1024, 1024
    oy, ox = cr.select_positions(oh, ow, persistent=True, fill=64, seed=1)
    key = set((oy * ow + ox).tolist())
    assert len(key) == len(oy), "duplicates"
    for r_ in (0, 1, oh - 2, oh - 1):
        assert all(r_ * ow + c in key for c in range(ow))
    for c in (0, 1, ow - 2, ow - 1):
        assert all(r_ * ow + c in key for r_ in range(oh))
    rows, cols = set(oy.tolist()), set(ox.tolist())
    for p in (4, 8, 32):
        assert all(m - 1 in rows and m in rows for m in range(p, oh, p))
    for p in (16, 32):
        assert all(m - 1 in cols and m in cols for m in range(p, ow, p))
    seam_cols = cr.seam_indices(ow, cr.COL_SEAMS)
    for L in (4, 8, 16, 32):                                 # both sides of every vertical strip end, at every seam column
        for m in range(4 * L, oh, 4 * L):
            assert all((m - 1) * ow + c in key and m * ow + c in key for c in seam_cols), L
    for L in (4, 8, 16, 32):                                 # horizontal strip ends: both sides of the column, at every seam row of a 16-row period
        for m in range(32 * L, ow, 32 * L):
            assert all(r_ * ow + m - 1 in key and r_ * ow + m in key for r_ in cr.seam_indices(oh, [16]))
    # shrinking the fill drops nothing else
    oy0, ox0 = cr.select_positions(oh, ow, persistent=True, fill=0, seed=1)
    assert set((oy0 * ow + ox0).tolist()) <= key and len(oy0) >= len(oy) - 64
    # small and odd maps, the transposed conv's 2h+1 grid
    for (a, b) in [(1, 1), (2, 3), (5, 33), (65, 65), (129, 1025)]:
        oy, ox = cr.select_positions(a, b, fill=16)
        assert oy.min() >= 0 and oy.max() < a and ox.min() >= 0 and ox.max() < b
        assert {0, a - 1} <= set(oy.tolist()) and {0, b - 1} <= set(ox.tolist())
    assert cr.select_channels(32) [0] == 0 and cr.select_channels(32)[-1] == 31 and len(cr.select_channels(32)) == 3
    ch = cr.select_channels(72)
    assert {0, 31, 32, 63}.issubset(ch) and set(range(64, 72)).issubset(ch) and len(ch) == 3 + 3 + 8
    assert cr.select_channels(3) == [0, 1, 2]
    assert cr.select_samples(1) == [0] and cr.select_samples(2) == [0, 1] and cr.select_samples(32) == [0, 1, 31]
    assert cr.seam_indices(9, [4]) == [3, 4, 7, 8] and cr.border_indices(3) == [0, 1, 2]


def test_strip_rule_matches_the_launch_code_cases():
    """1024^2, cin 32: one image walks vertical strips of 4 tiles, 2 / 4 / 8 images 8 / 16 / 32 (csrc/wino3.hip's own rule)."""
    assert [cr.wino3_strip(n, 32, 32, 1024, 1024) for n in (1, 2, 4, 8, 32)] == [("vertical", 4), ("vertical", 8), ("vertical", 16), ("vertical", 32),
                                                                                  ("vertical", 32)]
    assert cr.wino3_strip(1, 64, 64, 512, 512) is None and cr.wino3_strip(1, 32, 32, 64, 64) is None


class _FakeConv:
    """Stands for morphganformer_amd.conv: the seven wrappers with their real signatures, nothing launched."""

    def __init__(self):
        from morphganformer_amd import conv as cv
        self.calls = []
        for name in cr.WRAPPERS:
            setattr(self, name, self._make(name, getattr(cv, name)))

    def _make(self, name, real):
        import functools

        @functools.wraps(real)
        def fn(*a, **k):
            self.calls.append(name)
            if name == "winograd_forward":
                return self.winograd2_forward(a[0], a[1])         # delegates like the real one: still ONE record
            return None
        return fn


def test_recorder_deduplicates_and_records_outermost_calls_only():
    from morphganformer_amd import _lib
    from morphganformer_amd.conv import PackedConv
    fake = _FakeConv()
    originals = {n: getattr(fake, n) for n in cr.WRAPPERS}
    x = torch.zeros(2, 8, 16, 16)
    pc = PackedConv(torch.zeros(9, 8, 32), None, 20, 8, 3, 3, 32)
    u = torch.zeros(16, 2, 32, 4)
    ep = _lib.Epilogue(1, 0, 0, 1, 3, 0.2, 1.5, 0)
    with cr.Recorder(fake, profile=False) as rec:
        for _ in range(3):
            fake.conv_forward(x, pc, pad=(1, 1), epilogue=ep)
        fake.conv_forward(x, pc, pad=(1, 1))                                           # no epilogue: another record
        fake.conv_forward(torch.zeros(3, 8, 16, 16), pc, pad=(1, 1), epilogue=ep)      # another batch: another record
        fake.conv_forward(x, pc, (1), (1, 1), None, None, ep)                          # positional spelling of the first: the same record
        fake.winograd_forward(x, u)
        fake.winograd_forward(x, u, in_scale=torch.zeros(2, 8))
        fake.tconv3x3s2_forward(x, pc, out=torch.zeros(2, 20, 33, 36))
        fake.tconv3x3s2_forward(x, pc, out=torch.zeros(2, 20, 33, 64))                 # another pitch: another record
    assert rec.calls == 10 and len(rec.records) == 7 and not rec.conflicts
    assert fake.calls.count("winograd2_forward") == 2                                  # called through, not recorded
    names = sorted(dict(s)["wrapper"] for s in rec.records)
    assert names == ["conv_forward"] * 3 + ["tconv3x3s2_forward"] * 2 + ["winograd_forward"] * 2
    assert all(getattr(fake, n) is originals[n] for n in cr.WRAPPERS), "the wrappers are restored"
    one = dict(next(s for s in rec.records if dict(s)["wrapper"] == "conv_forward" and dict(s)["epilogue"] and dict(s)["x"][0] == 2))
    assert one["epilogue"] == (True, False, False, 1, 3, 0.2, 1.5, False) and one["weight"] == ("packed", 20, 8, 3, 3, 32) and one["pad"] == (1, 1)
    for s in rec.records:                                                              # a record holds no tensor
        assert "tensor(" not in repr(s).replace("'tensor'", "")


def test_bias_in_the_running_sum_and_the_masked_adjoint():
    """bias_in_sum adds |bias| to the denominator (a kernel whose accumulator starts at the bias rounds relative to it) and changes no value; the
    MDF adjoint's mask multiplies value and denominator by phi'(a) on its ring and makes both exactly 0 outside it.  The defects are still
    flagged with the larger denominator."""
    spec, _ = _layer(3, 32, 64, "corr", low=False)
    spec = spec.copy(noise=None, strength=None, act="relu", gain=1.0)
    n_sel, c_sel, oy, ox = _sel(spec)
    v0, a0 = cr.evaluate(spec, n_sel, c_sel, oy, ox)
    v1, a1 = cr.evaluate(spec.copy(bias_in_sum=True), n_sel, c_sel, oy, ox)
    assert torch.equal(v0, v1)
    assert float((a1 - a0 - spec.bias.double()[c_sel].abs()[None, :, None]).abs().max()) <= 1e-12
    res, _ = _gate(spec.copy(bias_in_sum=True), _zero_w(spec.copy(bias_in_sum=True), taps=4), lambda n, c, oy_, ox_: ox_ == spec.ow - 1)
    assert not res["ok"]
    res, _ = _gate(spec.copy(bias_in_sum=True), None)
    assert res["ok"]
    g = torch.Generator().manual_seed(9)
    a = torch.randn(spec.n, spec.cout, spec.oh, spec.ow, generator=g)
    plain = spec.copy(bias=None, act="linear")
    masked = plain.copy(mask=(a, 2, 0.2))
    vp, ap = cr.evaluate(plain, n_sel, c_sel, oy, ox)
    vm, am = cr.evaluate(masked, n_sel, c_sel, oy, ox)
    oyt, oxt = torch.as_tensor(oy), torch.as_tensor(ox)
    inside = ((oyt >= 2) & (oyt < spec.oh - 2) & (oxt >= 2) & (oxt < spec.ow - 2)).double()
    f = torch.where(a[n_sel][:, c_sel][:, :, oyt, oxt] > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.2, dtype=torch.float64)) * inside
    assert torch.equal(vm, vp * f) and torch.equal(am, ap * f) and bool((vm[..., inside == 0] == 0).all())
    # an adjoint that leaks a value outside its ring is flagged even where the reference is exactly 0
    leak = vm.clone().float()
    leak[..., (inside == 0).nonzero()[0]] = 1e-6
    c, _ = cr.gate_constant(vm.float(), vm, am, plain.products, cr.M_WINOGRAD)
    assert cr.compare(vm.float(), vm, am, c)["ok"] and not cr.compare(leak, vm, am, c)["ok"]
