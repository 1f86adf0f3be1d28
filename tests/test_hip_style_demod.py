"""The style / demodulation kernels (csrc/latent_prep.hip) and their adjoint (style_demod_bwd_body, csrc/backward.hip) in every launch
form, per element against the float64 formulas of tests/style_demod_cases.py.

Forward, mgf_style_demod_multi: the per-sample kernel, the batched kernel (all samples in one workgroup, n * max_cin floats of dynamic
LDS) at and below 64 KiB and above it (behind hipFuncSetAttribute, up to 128 KiB), and the fall-backs to the per-sample kernel at n > 32
and above 128 KiB; mgf_style_demod, the single-job entry.  Backward, mgf_style_demod_bwd_multi / mgf_latent_bwd_multi: the float4 slice
form and the scalar fallback of the demodulation product, the per-row chunk sums by one lane (< 16 chunks), by a wave (>= 16) and over
more than 64 chunks, demodulation switched off by each null pointer.  Operator level: mgf_demod_f32 past its 1024-block grid cap,
mgf_demod_bwd_f32 with a ragged second block.

Every operand is a guarded buffer, every output NaN-prefilled and guarded (tests/guarded_buffers.py); all are 16-byte aligned, as the
engine's are.  Every multi-sample case carries a sample with styles near 1e-3 (the 1e-8 inside the rsqrt is 1 % of the demodulation sum:
another constant there fails) and one with s = 0, d = 1e4.

Gates, all DOT_TOL = 1e-5 (tests/test_style_demod_host.py holds a float32 evaluation of the references below a quarter of it):
s against the sum of the absolute values of the element's terms, d per element, dwg and ds_op against the largest reference element of the
SAMPLE's row.  Run with -s for the measured maxima."""
import ctypes as C

import pytest
import torch

import latent_count_cases as lc
import style_demod_cases as sd
from guarded_buffers import NAN, device_table, g_in, g_out, rel

pytestmark = pytest.mark.gpu

DOT_TOL = sd.DOT_TOL


def _lib_():
    from morphganformer_amd import _lib
    return _lib, _lib.lib()


def _per_sample(got, ref, scale):
    """-> [n] float64: the largest |got - ref| / scale of each sample (an element whose scale is 0 must be exact)."""
    got, ref = got.detach().double().cpu(), ref.double()
    err = (got - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / scale).reshape(ref.shape[0], -1).amax(1)


def _gate(what, case, per_sample):
    print(f"[measured] {what} {case}: max {float(per_sample.max()):.2e}")
    bad = [i for i, e in enumerate(per_sample.tolist()) if not e < DOT_TOL]
    assert not bad, (what, case, "samples over the gate:", bad, [f"{per_sample[i]:.2e}" for i in bad])


# ================================================================================================ forward
class _FwdJob:
    """The guarded operands and outputs of one style job and its record."""

    def __init__(self, _lib, j, n):
        self.j = j
        self.aff_w, self.aff_b = g_in(j["aff_w"]), g_in(j["aff_b"])
        self.wsq = g_in(j["wsq"]) if j["demod"] else None
        self.s = g_out(n, j["cin"])
        self.d = g_out(n, j["cout"]) if j["demod"] else None
        self.rec = _lib.StyleJob(self.aff_w.ptr(), self.aff_b.ptr(), self.wsq.ptr() if self.wsq else 0, self.s.ptr(),
                                 self.d.ptr() if self.d else 0, j["cin"], j["cout"], j["w_offset"], j["aff_gain"], j["style_gain"])
        assert all(p % 16 == 0 for p in (self.rec.aff_w, self.rec.aff_b, self.rec.wsq or 0, self.rec.s, self.rec.d or 0))

    def outputs(self):
        return [o for o in (self.s, self.d) if o is not None]

    def check(self, ws, case):
        for o in self.outputs():
            assert o.written() and o.guard_intact(), case
        s_ref, sabs = sd.styles_ref(ws, self.j)
        _gate("s", case, _per_sample(self.s.t, s_ref, sabs))
        if self.d is not None:
            d_ref = sd.demod_ref(s_ref, self.j["wsq"])
            _gate("d", case, _per_sample(self.d.t, d_ref, d_ref))

    def snapshot_and_clear(self):
        snap = [o.t.clone() for o in self.outputs()]
        for o in self.outputs():
            o.t.fill_(NAN)
        return snap


@pytest.mark.parametrize("cid", list(sd.FORWARD_CASES))
def test_style_demod_multi_every_form_vs_float64(cid):
    """mgf_style_demod_multi, one table per case with a job without demodulation (the ToRGB layers) in it.  A0 / A64 (n = 1), B0 (max_cin
    unknown), F (n = 33) and G (17 x 2048 floats, more than 128 KiB) run the per-sample kernel; B64, C (exactly 64 KiB), D (68 KiB) and
    E (exactly 128 KiB) the styles-only launch and the batched kernel, D and E behind the raised dynamic-LDS limit."""
    _lib, L = _lib_()
    n, _jobs, max_cin = sd.FORWARD_CASES[cid]
    ws64, stride, jobs = sd.forward_case(cid)
    ws = g_in(ws64)
    fj = [_FwdJob(_lib, j, n) for j in jobs]
    table = device_table([f.rec for f in fj], _lib.StyleJob)
    call = lambda: _lib.check(L.mgf_style_demod_multi(table.data_ptr(), len(fj), ws.ptr(), stride, n, sd.WDIM, max_cin, _lib.stream_ptr()))
    call()
    for i, f in enumerate(fj):
        f.check(ws64, f"{cid} job {i} {(f.j['cin'], f.j['cout'])}")
    first = [f.snapshot_and_clear() for f in fj]
    call()                                                             # a fixed summation order: the same bits
    for f, snap in zip(fj, first):
        for o, before in zip(f.outputs(), snap):
            assert torch.equal(o.t, before) and o.guard_intact(), cid


@pytest.mark.parametrize("n,cin,cout", sd.SINGLE_JOB_CASES)
def test_style_demod_single_job_vs_float64(n, cin, cout):
    """mgf_style_demod: the job record by value, 16 blocks per sample; cout = 6 < 16 blocks, cin = 2048 fills the styles' LDS."""
    _lib, L = _lib_()
    ws64, stride, j = sd.single_job_case(n, cin, cout)
    ws, f = g_in(ws64), _FwdJob(_lib, j, n)
    call = lambda: _lib.check(L.mgf_style_demod(C.byref(f.rec), ws.ptr(), stride, n, sd.WDIM, _lib.stream_ptr()))
    call()
    f.check(ws64, f"single {(n, cin, cout)}")
    first = f.snapshot_and_clear()
    call()
    for o, before in zip(f.outputs(), first):
        assert torch.equal(o.t, before) and o.guard_intact()


def test_style_demod_refuses_more_than_2048_input_channels():
    """The styles of a job go to 2048 floats of LDS: the single-job entry refuses cin = 2049, the multi entry max_cin = 2049 (with
    max_cin = 0 the limit is the caller's to keep, include/mgf.h)."""
    _lib, L = _lib_()
    ws64, stride, j = sd.single_job_case(1, 20, 100)
    ws, f = g_in(ws64), _FwdJob(_lib, j, 1)
    f.rec.cin = 2049
    with pytest.raises(_lib.MgfError, match="2048"):
        _lib.check(L.mgf_style_demod(C.byref(f.rec), ws.ptr(), stride, 1, sd.WDIM, _lib.stream_ptr()))
    f.rec.cin = 20
    table = device_table([f.rec], _lib.StyleJob)
    with pytest.raises(_lib.MgfError, match="2048"):
        _lib.check(L.mgf_style_demod_multi(table.data_ptr(), 1, ws.ptr(), stride, 1, sd.WDIM, 2049, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(f.s.t).all()) and bool(torch.isnan(f.d.t).all())           # nothing was launched


# ================================================================================================ backward
class _BwdJob:
    def __init__(self, _lib, job, off=()):
        """off: the names among wsq, d, dc_part whose pointer the record leaves null."""
        self.job = job
        self.bufs = {k: g_in(job[k]) for k in ("aff_w", "wsq", "s", "d", "ds_part", "dc_part")}
        p = {k: (0 if k in off else b.ptr()) for k, b in self.bufs.items()}
        assert all(v % 16 == 0 for v in p.values())
        self.rec = _lib.StyleBwdJob(p["aff_w"], p["wsq"], p["s"], p["d"], p["ds_part"], p["dc_part"], job["cin"], job["cout"],
                                    job["s_chunks"], job["d_chunks"], job["aff_gain"], job["style_gain"])


def _run_style_bwd(_lib, L, recs, n, wdim, max_channels, fused):
    table = device_table(recs, _lib.StyleBwdJob)
    dwg = g_out(n, len(recs), wdim)
    if fused:
        _lib.check(L.mgf_latent_bwd_multi(dwg.ptr(), table.data_ptr(), len(recs), None, None, 0, n, 1, wdim, max_channels, _lib.stream_ptr()))
    else:
        _lib.check(L.mgf_style_demod_bwd_multi(dwg.ptr(), table.data_ptr(), len(recs), n, wdim, max_channels, _lib.stream_ptr()))
    assert dwg.written() and dwg.guard_intact()
    return dwg


@pytest.mark.parametrize("n,cin,cout,sc,dc", sd.BACKWARD_CASES)
def test_style_demod_bwd_every_form_vs_float64(n, cin, cout, sc, dc):
    """dwg with demodulation: cin = 4, 64, 512, 1024 take the float4 slice form of sum_o tl[o] wsq[o][i] (1, 16, 128, 256 lanes across
    the channels), 20, 48, 768, 2048 the scalar fallback; the chunk sums run by one lane (1, 2, 15), by a wave (16, 17) and twice over
    the lanes (70).  s and d are the float64 references rounded to float32."""
    _lib, L = _lib_()
    job = sd.bwd_job(n, cin, cout, sc, dc)
    _ds, dwg_ref = sd.style_bwd_ref(job, True)
    bj = _BwdJob(_lib, job)
    mc = max(cin, cout)
    dwg = _run_style_bwd(_lib, L, [bj.rec], n, sd.WDIM, mc, fused=False)
    _gate("dwg", (n, cin, cout, sc, dc), _per_sample(dwg.t[:, 0], dwg_ref, dwg_ref.abs().amax(1, keepdim=True)))
    # the fused entry without attention jobs, and a second call: the same bits
    assert torch.equal(_run_style_bwd(_lib, L, [bj.rec], n, sd.WDIM, mc, fused=True).t, dwg.t)
    assert torch.equal(_run_style_bwd(_lib, L, [bj.rec], n, sd.WDIM, mc, fused=False).t, dwg.t)


@pytest.mark.parametrize("way", sd.DEMOD_OFF_WAYS)
def test_style_demod_bwd_without_demodulation_each_null_pointer(way):
    """Any of wsq, d, dc_part null switches the second term off: the result is the gradient of the styles alone."""
    _lib, L = _lib_()
    n, cin, cout, sc, dc = sd.DEMOD_OFF_CASE
    job = sd.bwd_job(n, cin, cout, sc, dc)
    _ds, dwg_ref = sd.style_bwd_ref(job, False)
    assert rel(dwg_ref, sd.style_bwd_ref(job, True)[1]) > 0.1          # (the term that is switched off is not small)
    off = ("wsq", "d", "dc_part") if way == "all" else (way,)
    bj = _BwdJob(_lib, job, off)
    dwg = _run_style_bwd(_lib, L, [bj.rec], n, sd.WDIM, max(cin, cout), fused=False)
    _gate("dwg", ("no demodulation", way), _per_sample(dwg.t[:, 0], dwg_ref, dwg_ref.abs().amax(1, keepdim=True)))
    assert torch.equal(_run_style_bwd(_lib, L, [bj.rec], n, sd.WDIM, max(cin, cout), fused=True).t, dwg.t)


def test_style_demod_bwd_at_latent_width_64():
    """wdim = 64: four slices of the input channels meet in the final reduce instead of eight."""
    _lib, L = _lib_()
    n, cin, cout, sc, dc = sd.WDIM64_CASE
    job = sd.bwd_job(n, cin, cout, sc, dc, wdim=64)
    _ds, dwg_ref = sd.style_bwd_ref(job, True)
    bj = _BwdJob(_lib, job)
    dwg = _run_style_bwd(_lib, L, [bj.rec], n, 64, max(cin, cout), fused=False)
    _gate("dwg", ("wdim 64",) + sd.WDIM64_CASE, _per_sample(dwg.t[:, 0], dwg_ref, dwg_ref.abs().amax(1, keepdim=True)))
    assert torch.equal(_run_style_bwd(_lib, L, [bj.rec], n, 64, max(cin, cout), fused=True).t, dwg.t)


def test_latent_bwd_multi_demodulated_jobs_next_to_attention_jobs():
    """One mgf_latent_bwd_multi launch as grad.py issues it: three demodulated style jobs (float4 form, fallback, 70 chunks), one without
    demodulation and two attention jobs (tests/latent_count_cases.py, T = 5) -- dwg [n, job, wdim] by job index, dyc untouched by them."""
    _lib, L = _lib_()
    n, T, D = 3, 5, sd.WDIM
    jobs = [sd.bwd_job(n, cin, cout, sc, dc) for (cin, cout, sc, dc) in sd.MIXED_JOBS]
    plain = sd.bwd_job(n, 20, 3, 3, 1)
    bjs = [_BwdJob(_lib, j) for j in jobs] + [_BwdJob(_lib, plain, ("wsq", "d", "dc_part"))]
    refs = [sd.style_bwd_ref(j, True)[1] for j in jobs] + [sd.style_bwd_ref(plain, False)[1]]
    cs = (20, 64)
    inp = lc.latent_side_inputs(T, cs, n=n)
    _vwb, dyc_ref, _dwg, _dw = lc.latent_side_ref(inp, 1.0)
    wmv, dvwb = [g_in(w) for w in inp["wmv"]], [g_in(d, 16) for d in inp["dvwb"]]
    atable = device_table([_lib.AttnBwdJob(wmv[j].ptr(), dvwb[j].ptr(), cs[j], 0) for j in range(2)], _lib.AttnBwdJob)
    stable = device_table([b.rec for b in bjs], _lib.StyleBwdJob)

    def run():
        dwg, dyc = g_out(n, len(bjs), D), g_out(n, 2, T, D)
        _lib.check(L.mgf_latent_bwd_multi(dwg.ptr(), stable.data_ptr(), len(bjs), dyc.ptr(), atable.data_ptr(), 2, n, T, D, 768, _lib.stream_ptr()))
        assert dwg.written() and dwg.guard_intact() and dyc.written() and dyc.guard_intact()
        return dwg, dyc
    dwg, dyc = run()
    for i, want in enumerate(refs):
        _gate("dwg", f"mixed launch job {i}", _per_sample(dwg.t[:, i], want, want.abs().amax(1, keepdim=True)))
    assert rel(dyc.t, dyc_ref) < DOT_TOL
    dwg2, dyc2 = run()
    assert torch.equal(dwg2.t, dwg.t) and torch.equal(dyc2.t, dyc.t)
    # the style jobs alone: the same bits as next to the attention jobs
    assert torch.equal(_run_style_bwd(_lib, L, [b.rec for b in bjs], n, D, 768, fused=False).t, dwg.t)


def test_style_demod_bwd_refuses_width_48_and_2049_channels():
    _lib, L = _lib_()
    job = sd.bwd_job(1, 4, 3, 1, 1)
    bj = _BwdJob(_lib, job)
    table = device_table([bj.rec], _lib.StyleBwdJob)
    dwg = g_out(1, 1, 64)
    st = _lib.stream_ptr()
    with pytest.raises(_lib.MgfError, match="wdim must divide 256"):
        _lib.check(L.mgf_style_demod_bwd_multi(dwg.ptr(), table.data_ptr(), 1, 1, 48, 4, st))
    with pytest.raises(_lib.MgfError, match="wdim must divide 256"):
        _lib.check(L.mgf_latent_bwd_multi(dwg.ptr(), table.data_ptr(), 1, None, None, 0, 1, 1, 48, 4, st))
    with pytest.raises(_lib.MgfError, match="at most 2048 channels"):
        _lib.check(L.mgf_style_demod_bwd_multi(dwg.ptr(), table.data_ptr(), 1, 1, sd.WDIM, 2049, st))
    with pytest.raises(_lib.MgfError, match="at most 2048 channels"):
        _lib.check(L.mgf_latent_bwd_multi(dwg.ptr(), table.data_ptr(), 1, None, None, 0, 1, 1, sd.WDIM, 2049, st))
    torch.cuda.synchronize()
    assert bool(torch.isnan(dwg.t).all())


# ================================================================================================ operator level
@pytest.mark.parametrize("n,cin,cout,roles", sd.DEMOD_OP_CASES)
def test_demod_f32_vs_float64(n, cin, cout, roles):
    """mgf_demod_f32: 4100 rows are more than the 1024 blocks of 4 waves the grid is capped at hold, so block 0 takes a second trip
    (rows 4096 .. 4099); cout = 3 and 1 leave waves without a row."""
    _lib, L = _lib_()
    inp = sd.demod_op_inputs(n, cin, cout, roles)
    d_ref = sd.demod_ref(inp["s"], inp["wsq"])
    s, wsq = g_in(inp["s"]), g_in(inp["wsq"])
    outs = []
    for _ in range(2):
        d = g_out(n, cout)
        _lib.check(L.mgf_demod_f32(d.ptr(), s.ptr(), wsq.ptr(), n, cin, cout, _lib.stream_ptr()))
        assert d.written() and d.guard_intact()
        outs.append(d)
    _gate("d (operator)", (n, cin, cout), _per_sample(outs[0].t, d_ref, d_ref))
    assert torch.equal(outs[0].t, outs[1].t)


@pytest.mark.parametrize("n,cin,cout,roles", sd.DEMOD_BWD_OP_CASES)
def test_demod_bwd_f32_vs_float64(n, cin, cout, roles):
    """mgf_demod_bwd_f32, one lane per input channel: 257 channels are two blocks, the second with one lane at work."""
    _lib, L = _lib_()
    inp = sd.demod_op_inputs(n, cin, cout, roles)
    ref = sd.demod_bwd_ref(inp["dd"], inp["d"], inp["s"], inp["wsq"])
    s, wsq, d, dd = g_in(inp["s"]), g_in(inp["wsq"]), g_in(inp["d"]), g_in(inp["dd"])
    outs = []
    for _ in range(2):
        ds = g_out(n, cin)
        _lib.check(L.mgf_demod_bwd_f32(ds.ptr(), dd.ptr(), d.ptr(), s.ptr(), wsq.ptr(), n, cin, cout, _lib.stream_ptr()))
        assert ds.written() and ds.guard_intact()
        outs.append(ds)
    _gate("ds (operator)", (n, cin, cout), _per_sample(outs[0].t, ref, ref.abs().amax(1, keepdim=True)))
    assert torch.equal(outs[0].t, outs[1].t)
