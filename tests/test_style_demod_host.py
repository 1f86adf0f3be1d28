"""CPU: the references and the gates of tests/test_hip_style_demod.py, on the references alone.

1. The float64 adjoints of tests/style_demod_cases.py (dwg of a style-gradient job, ds_op of the operator-level demodulation) equal torch
   autograd of the forward formulas in float64 to 1e-12: they are tied to the operation, not to a header comment.
2. The same formulas evaluated in float32 -- every product and every partial sum rounded to float32 -- stay below a QUARTER of the gate
   (DOT_TOL = 1e-5) on the inputs of every case: the gate the kernels must meet is 4x what single precision costs the reference itself.
   A case that misses the quarter gets other inputs, never another gate.
"""
import pytest
import torch

import style_demod_cases as sd

QUARTER = sd.DOT_TOL / 4


# ================================================================================================ 1. the adjoints are autograd's
@pytest.mark.parametrize("n,cin,cout,sc,dc", sd.BACKWARD_CASES + [sd.WDIM64_CASE])
def test_style_gradient_reference_is_autograd_of_the_forward_formulas(n, cin, cout, sc, dc):
    """dwg = d/dwg [ sum_i DS_i s_i(wg) + sum_o stopgrad(a_o / d_o) d_o(wg) ] with DS = sum_chunks ds_part and a = sum_chunks dc_part (the
    layer's output is c_o = d_o (...), so <dc_o, c_o> / d_o is what multiplies d d_o)."""
    wdim = 64 if (n, cin, cout, sc, dc) == sd.WDIM64_CASE else sd.WDIM
    job = sd.bwd_job(n, cin, cout, sc, dc, wdim=wdim)
    wg = job["wg"].clone().requires_grad_(True)
    s = wg @ job["aff_w"].T * job["aff_gain"] * job["style_gain"]
    d = sd.demod_ref(s, job["wsq"])
    DS, a = job["ds_part"].sum(-1), job["dc_part"].sum(-1)
    (want,) = torch.autograd.grad((DS * s).sum() + ((a / d).detach() * d).sum(), wg, retain_graph=True)
    ds, dwg = sd.style_bwd_ref(job, True, s.detach(), d.detach())
    assert sd.rows_rel(dwg, want) < 1e-12
    # without demodulation: the first term alone
    (want0,) = torch.autograd.grad((DS * s).sum(), wg)
    assert sd.rows_rel(sd.style_bwd_ref(job, False, s.detach(), d.detach())[1], want0) < 1e-12
    # the rounded s and d the kernels are handed move the reference by float32 rounding, far inside the gate
    assert sd.rows_rel(sd.style_bwd_ref(job)[1], dwg) < 1e-6


@pytest.mark.parametrize("n,cin,cout,roles", sd.DEMOD_OP_CASES + sd.DEMOD_BWD_OP_CASES)
def test_demod_adjoint_reference_is_autograd(n, cin, cout, roles):
    inp = sd.demod_op_inputs(n, cin, cout, roles)
    s = inp["s"].clone().requires_grad_(True)
    d = sd.demod_ref(s, inp["wsq"])
    (want,) = torch.autograd.grad((inp["dd"] * d).sum(), s)
    assert sd.rows_rel(sd.demod_bwd_ref(inp["dd"], d.detach(), inp["s"], inp["wsq"]), want) < 1e-12


# ================================================================================================ the cases are what they claim
def test_sample_roles_small_and_zero_styles():
    """In every multi-sample case a demodulated job with aff_b = 0 has a sample whose 1e-8 is about 1 % of the demodulation sum and a
    sample with s = 0, d = 1e4."""
    for cid, (n, jobs, max_cin) in sd.FORWARD_CASES.items():
        ws, stride, js = sd.forward_case(cid)
        assert stride == sd.SLOTS * sd.WDIM and all(j["w_offset"] > 0 for j in js)
        assert any(not j["demod"] for j in js), cid
        assert max(j["cin"] for j in js) == (max_cin or max(j["cin"] for j in js))
        if n < 3:
            continue
        hit = 0
        for j in js:
            if not j["demod"] or bool(j["aff_b"].abs().max() > 0):
                continue
            s, _ = sd.styles_ref(ws, j)
            acc = s.square() @ j["wsq"].T
            assert 1e-7 < float(acc[1].min()) and float(acc[1].max()) < 1e-5, (cid, float(acc[1].min()), float(acc[1].max()))
            assert bool((s[n - 1] == 0).all()) and float((sd.demod_ref(s, j["wsq"])[n - 1] - 1e4).abs().max()) < 1e-6
            hit += 1
        assert hit >= 1, cid
    for (n, cin, cout, sc, dc) in sd.BACKWARD_CASES:
        job = sd.bwd_job(n, cin, cout, sc, dc)
        if n >= 3:
            assert float(job["s"][1].abs().max()) < 1e-2 and bool((job["s"][2] == 0).all()) and float((job["d"][2] - 1e4).abs().max()) < 1e-3


def test_forward_cases_reach_the_forms_they_name():
    """The dispatch rule of mgf_style_demod_multi (csrc/latent_prep.hip) written out: batched when 1 < n <= 32, max_cin known and
    n * max_cin floats <= 128 KiB; the dynamic-LDS limit is raised above 64 KiB."""
    lds = {cid: 4 * n * max_cin for cid, (n, _jobs, max_cin) in sd.FORWARD_CASES.items()}
    batched = tuple(cid for cid, (n, _jobs, max_cin) in sd.FORWARD_CASES.items() if 1 < n <= 32 and max_cin > 0 and lds[cid] <= 128 << 10)
    assert batched == sd.BATCHED_FORWARD
    assert lds["C"] == 64 << 10 and 64 << 10 < lds["D"] < 128 << 10 and lds["E"] == 128 << 10 and lds["G"] > 128 << 10
    assert lds["B64"] < 64 << 10 and sd.FORWARD_CASES["F"][0] == 33 and sd.FORWARD_CASES["B0"][2] == 0
    assert all(j[0] <= 2048 for _n, jobs, _m in sd.FORWARD_CASES.values() for j in jobs)


def test_backward_cases_cover_every_value_and_form():
    cases = sd.BACKWARD_CASES
    float4 = lambda c: c % 4 == 0 and c // 4 <= 256 and 256 % (c // 4) == 0
    assert {c[1] for c in cases} == set(sd.FLOAT4_CIN) | set(sd.FALLBACK_CIN)
    assert all(float4(c) for c in sd.FLOAT4_CIN) and not any(float4(c) for c in sd.FALLBACK_CIN)
    assert {c[2] for c in cases} == {3, 100, 2048} and {c[0] for c in cases} == {1, 3}
    assert {(c[3], c[4]) for c in cases} == {(1, 1), (15, 17), (16, 15), (70, 16), (2, 70)}
    assert all(c[1] * c[2] * 4 <= 8 << 20 for c in cases)
    for form in (sd.FLOAT4_CIN, sd.FALLBACK_CIN):                     # each form sees demodulation sums over < 16, 16..64 and > 64 chunks
        dcs = {c[4] for c in cases if c[1] in form}
        assert min(dcs) < 16 and any(16 <= x <= 64 for x in dcs) and max(dcs) > 64, dcs


# ================================================================================================ 2. the gate is 4x float32
def _show(what, case, **figures):
    print(f"[float32] {what} {case}: " + "  ".join(f"{k} {v:.2e}" for k, v in figures.items()))


@pytest.mark.parametrize("cid", [c for c in sd.FORWARD_CASES if c not in ("A64", "B0")])      # (the same operands as A0 / B64)
def test_float32_forward_is_within_a_quarter_of_the_gate(cid):
    ws, stride, jobs = sd.forward_case(cid)
    for i, j in enumerate(jobs):
        s, sabs = sd.styles_ref(ws, j)
        es = sd.scaled_err(sd.styles_f32(ws, j), s, sabs)
        ed = 0.0
        if j["demod"]:
            d = sd.demod_ref(s, j["wsq"])
            ed = sd.scaled_err(sd.demod_f32(s, j["wsq"]), d, d)           # (from the float64 styles rounded once, as a kernel given s sees them)
            ed = max(ed, sd.scaled_err(sd.demod_f32(sd.styles_f32(ws, j), j["wsq"]), d, d))       # and from the float32 styles
        _show("forward", f"{cid} job {i}", s=es, d=ed)
        assert es < QUARTER and ed < QUARTER, (cid, i, es, ed)


@pytest.mark.parametrize("n,cin,cout", sd.SINGLE_JOB_CASES)
def test_float32_single_job_is_within_a_quarter_of_the_gate(n, cin, cout):
    ws, stride, j = sd.single_job_case(n, cin, cout)
    s, sabs = sd.styles_ref(ws, j)
    d = sd.demod_ref(s, j["wsq"])
    es, ed = sd.scaled_err(sd.styles_f32(ws, j), s, sabs), sd.scaled_err(sd.demod_f32(sd.styles_f32(ws, j), j["wsq"]), d, d)
    _show("single job", (n, cin, cout), s=es, d=ed)
    assert es < QUARTER and ed < QUARTER


@pytest.mark.parametrize("n,cin,cout,sc,dc", sd.BACKWARD_CASES + [sd.WDIM64_CASE])
def test_float32_style_gradient_is_within_a_quarter_of_the_gate(n, cin, cout, sc, dc):
    wdim = 64 if (n, cin, cout, sc, dc) == sd.WDIM64_CASE else sd.WDIM
    job = sd.bwd_job(n, cin, cout, sc, dc, wdim=wdim)
    for demod in (True, False):
        ds, dwg = sd.style_bwd_ref(job, demod)
        ds32, dwg32 = sd.style_bwd_f32(job, demod)
        e_ds, e_dwg = sd.rows_rel(ds32, ds), sd.rows_rel(dwg32, dwg)
        _show("style gradient", (n, cin, cout, sc, dc, "demod" if demod else "plain"), ds=e_ds, dwg=e_dwg)
        assert e_ds < QUARTER and e_dwg < QUARTER


@pytest.mark.parametrize("n,cin,cout,roles", sd.DEMOD_OP_CASES + sd.DEMOD_BWD_OP_CASES)
def test_float32_operator_level_is_within_a_quarter_of_the_gate(n, cin, cout, roles):
    inp = sd.demod_op_inputs(n, cin, cout, roles)
    d = sd.demod_ref(inp["s"], inp["wsq"])
    ed = sd.scaled_err(sd.demod_f32(inp["s"], inp["wsq"]), d, d)
    e_ds = sd.rows_rel(sd.demod_bwd_f32(inp["dd"], inp["d"], inp["s"], inp["wsq"]), sd.demod_bwd_ref(inp["dd"], inp["d"], inp["s"], inp["wsq"]))
    _show("operator", (n, cin, cout), d=ed, ds_op=e_ds)
    assert ed < QUARTER and e_ds < QUARTER
