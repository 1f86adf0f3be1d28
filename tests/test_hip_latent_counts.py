"""The attention kernels, the latent-side reductions, the generator, its gradient and a projection at latent counts other than k = 17.

Every other GPU test runs T = k - 1 = 16 local latents, where the kernels copy their [c][T] tables 16 bytes at a time, never mask a padded
latent and take the register-resident / MFMA forms.  T < 16 is another path through each of them (csrc/attention.hip, csrc/backward.hip,
csrc/latent_prep.hip) and other strides in every buffer engine.py / grad.py derive from cfg.k.  Part 1 calls the C entries directly
against the float64 formulas of tests/latent_count_cases.py; part 2 runs whole generators against the CPU oracle.

Direct calls hand the kernels GUARDED buffers (tests/guarded_buffers.py): an operand lies at the head of a larger NaN-filled allocation (a read with a wrong stride
pulls NaN into the result instead of a neighbour's plausible numbers, and stays inside the allocation), an output is NaN before the call and
is followed by a NaN guard that must still be NaN after it (a write with a wrong stride either leaves NaN inside or lands in the guard).

The argmax comparisons leave out pixels whose two best are within 1e-4; at most 3 % of a layer's pixels may be left out
(tests/test_latent_counts_host.py asserts that on the references alone, the tests here assert it again)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import latent_count_cases as lc
from guarded_buffers import NAN, Guarded, device_table as _device_table, g_in, g_out, rel

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3                       # the gradient gate of tests/test_hip_gradient.py
PIX_TOL = 1e-3                        # the pixel gate of tests/test_hip_generator.py
DOT_TOL = 1e-5                        # float32 dot-product kernels (channel_dot, style_grad): relative to the largest element


def _lib_():
    from morphganformer_amd import _lib
    return _lib, _lib.lib()


# ================================================================================================ 1. direct kernel calls
@pytest.mark.parametrize("n,c,f,T,with_ep", lc.FORWARD_CASES)
def test_duplex_attention_forward_latent_counts_vs_float64(n, c, f, T, with_ep):
    """mgf_duplex_attention at T = 1, 2, 5, 8, 15 (and the ragged-channel shape at T = 16): the padded table staging, the masked softmax
    and argmax, probs and spos with row stride T; (3, 64, 80) and (1, 256, 64) take the register-resident and the MFMA kernel at T = 16 and
    must not here, (1, 256, 4096) the 4-blocks-per-workgroup kernel; 16400 pixels run 64-pixel blocks, the last one ragged."""
    _lib, L = _lib_()
    inp = lc.attention_inputs(n, c, f, T)
    S, P, y = lc.attention_forward_ref(inp, with_ep)
    x, wq, sp, vw = g_in(inp["x"]), g_in(inp["wqc"], 16), g_in(inp["spos"], 16), g_in(inp["vwb"], 16)
    nz, bs, rs = g_in(inp["noise"]), g_in(inp["bias"]), g_in(inp["res"])
    st = torch.tensor([lc.EP_NOISE_STRENGTH], device="cuda")
    ep = _lib.make_epilogue(bias=bs.t, noise=nz.t, noise_strength=st, noise_n=n, act="lrelu", alpha=lc.EP_ALPHA, gain=lc.EP_GAIN,
                            residual=rs.t) if with_ep else None
    epp = C.byref(ep) if ep is not None else None
    out, probs, amax = g_out(n, c, f), g_out(n, f, T, span=16), g_out(n, f)
    am = amax.t.view(torch.int32)                          # (a NaN's bit pattern read as int32 is 2143289344: an unwritten entry fails `< T`)
    _lib.check(L.mgf_duplex_attention(out.ptr(), x.ptr(), wq.ptr(), sp.ptr(), vw.ptr(), n, c, f, T, epp, 0, probs.ptr(), am.data_ptr(),
                                      _lib.stream_ptr()))
    assert out.written() and probs.written()
    assert out.guard_intact() and probs.guard_intact() and amax.guard_intact()
    assert rel(out.t, y) < 2e-5
    assert float((probs.t.double().cpu() - P).abs().max()) < 1e-5
    assert float((probs.t.double().sum(-1) - 1).abs().max()) < 1e-5
    a = am.cpu().long()
    assert int(a.min()) >= 0 and int(a.max()) < T
    clear = lc.decided(S)
    assert 1.0 - float(clear.double().mean()) <= lc.MAX_UNDECIDED
    assert bool((a[clear] == S.argmax(-1)[clear]).all())
    if T == 1:
        assert bool((a == 0).all())
    # without the optional outputs: the same bits
    out2 = g_out(n, c, f)
    _lib.check(L.mgf_duplex_attention(out2.ptr(), x.ptr(), wq.ptr(), sp.ptr(), vw.ptr(), n, c, f, T, epp, 0, None, None, _lib.stream_ptr()))
    assert torch.equal(out.t, out2.t) and out2.guard_intact()


@pytest.mark.parametrize("n,c,res,T", lc.BACKWARD_CASES)
def test_duplex_attention_bwd_latent_counts_match_autograd(n, c, res, T):
    """mgf_duplex_attention_bwd + mgf_attn_values_grad[_ws] at T < 16 against autograd of the float64 layer; (1, 256, 8) takes the MFMA
    kernels at T = 16 and must fall through to the register ones here, (1, 512, 4) stages more than 64 KiB of tables."""
    _lib, L = _lib_()
    f = res * res
    inp = lc.attention_inputs(n, c, f, T)
    P, dx_ref, dv_ref = lc.attention_backward_ref(inp)
    x, da, wq, sp, vw = g_in(inp["x"]), g_in(inp["da"]), g_in(inp["wqc"], 16), g_in(inp["spos"], 16), g_in(inp["vwb"], 16)
    dx, dg, probs = g_out(n, c, f), g_out(n, c, f), g_out(n, f, T, span=16)
    _lib.check(L.mgf_duplex_attention_bwd(dx.ptr(), dg.ptr(), probs.ptr(), da.ptr(), x.ptr(), wq.ptr(), sp.ptr(), vw.ptr(), n, c, f, T,
                                          _lib.stream_ptr()))
    assert dx.written() and dg.written() and probs.written()
    assert dx.guard_intact() and dg.guard_intact() and probs.guard_intact()
    assert rel(probs.t, P) < 1e-4
    assert rel(dx.t, dx_ref) < GRAD_TOL
    r = torch.rsqrt(inp["x"].square().mean(1, keepdim=True) + 1e-8)
    assert rel(dg.t, inp["da"] * inp["x"] * r) < 1e-5                  # (the header's definition of the scratch the value gradient reads)
    dv = g_out(n, c, T, span=16)
    _lib.check(L.mgf_attn_values_grad(dv.ptr(), dg.ptr(), probs.ptr(), n, c, f, T, _lib.stream_ptr()))
    assert dv.written() and dv.guard_intact()
    assert rel(dv.t, dv_ref) < GRAD_TOL
    # no MFMA form below 16 latents: grad.py plans its deferred by-products around this answer, and the _ws entry falls back to the kernel above
    assert int(L.mgf_attn_values_grad_slices(n, c, f, T)) == 0
    ws = torch.full((int(L.mgf_attn_values_grad_workspace_floats(n, c)),), NAN, device="cuda")
    dv2, dv3 = g_out(n, c, T, span=16), g_out(n, c, T, span=16)
    for o in (dv2, dv3):
        _lib.check(L.mgf_attn_values_grad_ws(o.ptr(), dg.ptr(), probs.ptr(), n, c, f, T, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        assert o.written() and o.guard_intact()
    assert torch.equal(dv2.t, dv.t) and torch.equal(dv2.t, dv3.t)


@pytest.mark.parametrize("cs", lc.LATENT_CHANNELS)
@pytest.mark.parametrize("T", lc.LATENT_T)
def test_latent_side_reductions_vs_float64(T, cs):
    """mgf_attn_values / mgf_attn_values_multi (the value tables vwb), mgf_attn_values_bwd_multi and mgf_latent_bwd_multi (their gradient
    dyc, next to the style jobs' dwg) and mgf_latent_grad_gather (dw over k = T + 1 rows) against float64 einsums, with the job tables
    built the way engine.py and grad.py build them: one latent set [n, k, D] shared by all layers and per-layer latents [n, k, slots, D].

    Gate: 1e-5 of the largest element, the project's figure for float32 dot products (sums of at most 64 products here: a plain float32
    evaluation of the same sums is within 3e-7 of the float64 one)."""
    _lib, L = _lib_()
    n, D, k = lc.LATENT_N, lc.LATENT_WDIM, T + 1
    inp = lc.latent_side_inputs(T, cs)
    scale = 0.6
    vwb_ref, dyc_ref, dwg_ref, dw_ref = lc.latent_side_ref(inp, scale)
    st = _lib.stream_ptr()
    wmv, bmv = [g_in(w) for w in inp["wmv"]], [g_in(b) for b in inp["bmv"]]
    # ---- value tables: the shared latent set, through the device job table (engine.py: tables(False)) and one job at a time
    w = g_in(inp["w"])
    vw = [g_out(n, c, T, span=16) for c in cs]
    jobs = [_lib.AttnJob(wmv[j].ptr(), bmv[j].ptr(), vw[j].ptr(), cs[j], 0) for j in range(2)]
    table = _device_table(jobs, _lib.AttnJob)
    _lib.check(L.mgf_attn_values_multi(table.data_ptr(), 2, w.ptr(), k * D, D, n, T, D, st))
    for j in range(2):
        assert vw[j].written() and vw[j].guard_intact()
        assert rel(vw[j].t, vwb_ref[j]) < DOT_TOL, j
        one = g_out(n, cs[j], T, span=16)
        job = _lib.AttnJob(wmv[j].ptr(), bmv[j].ptr(), one.ptr(), cs[j], 0)
        _lib.check(L.mgf_attn_values(C.byref(job), w.ptr(), k * D, D, n, T, D, st))
        assert torch.equal(one.t, vw[j].t) and one.guard_intact()
    # ---- per-layer latents: layer `slot` reads ws[:, :, slot] (engine.py: tables(True)); slots 1 and 2 of 3 carry the latents above
    ws4 = torch.randn(n, k, 3, D, dtype=torch.float64)
    ws4[:, :, 1] = inp["w"]
    ws4[:, :, 2] = inp["w"]
    wsd = g_in(ws4)
    vw4 = [g_out(n, c, T, span=16) for c in cs]
    table4 = _device_table([_lib.AttnJob(wmv[j].ptr(), bmv[j].ptr(), vw4[j].ptr(), cs[j], (1 + j) * D) for j in range(2)], _lib.AttnJob)
    _lib.check(L.mgf_attn_values_multi(table4.data_ptr(), 2, wsd.ptr(), k * 3 * D, 3 * D, n, T, D, st))
    for j in range(2):
        assert torch.equal(vw4[j].t, vw[j].t) and vw4[j].guard_intact(), j
    # ---- a weight table 4 bytes off 16-byte alignment: include/mgf.h asks no alignment of mgf_attn_job.wmv, so the entry must compute
    off = Guarded((cs[0], D), inp["wmv"][0], offset=1)
    assert off.ptr() % 16 == 4
    vo = g_out(n, cs[0], T, span=16)
    job = _lib.AttnJob(off.ptr(), bmv[0].ptr(), vo.ptr(), cs[0], 0)
    _lib.check(L.mgf_attn_values(C.byref(job), w.ptr(), k * D, D, n, T, D, st))
    assert vo.written() and vo.guard_intact() and rel(vo.t, vwb_ref[0]) < DOT_TOL

    # ---- backward: dyc from the value-table gradients, alone and next to the style jobs (grad.py: _alloc)
    dvwb = [g_in(d, 16) for d in inp["dvwb"]]
    atable = _device_table([_lib.AttnBwdJob(wmv[j].ptr(), dvwb[j].ptr(), cs[j], 0) for j in range(2)], _lib.AttnBwdJob)
    dyc = g_out(n, 2, T, D)
    _lib.check(L.mgf_attn_values_bwd_multi(dyc.ptr(), atable.data_ptr(), 2, n, T, D, st))
    assert dyc.written() and dyc.guard_intact()
    assert rel(dyc.t, dyc_ref) < DOT_TOL
    sty = inp["style"]
    aff, dsp = [g_in(s["aff_w"]) for s in sty], [g_in(s["ds_part"]) for s in sty]
    s_dummy = torch.ones(n, 64, device="cuda")
    stable = _device_table([_lib.StyleBwdJob(aff[j].ptr(), 0, s_dummy.data_ptr(), 0, dsp[j].ptr(), 0, s["cin"], 8, s["chunks"], 1,
                                             s["aff_gain"], s["style_gain"]) for j, s in enumerate(sty)], _lib.StyleBwdJob)
    dwg, dyc2 = g_out(n, 2, D), g_out(n, 2, T, D)
    _lib.check(L.mgf_latent_bwd_multi(dwg.ptr(), stable.data_ptr(), 2, dyc2.ptr(), atable.data_ptr(), 2, n, T, D, 64, st))
    assert dwg.written() and dwg.guard_intact() and dyc2.written() and dyc2.guard_intact()
    assert torch.equal(dyc2.t, dyc.t)
    assert rel(dwg.t, dwg_ref) < DOT_TOL
    # ---- gather: rows t < T from the attention jobs, row T from the style jobs
    dw = g_out(n, k, D)
    _lib.check(L.mgf_latent_grad_gather(dw.ptr(), dwg.ptr(), 2, dyc.ptr(), 2, n, k, D, scale, st))
    assert dw.written() and dw.guard_intact()
    assert rel(dw.t, dw_ref) < DOT_TOL
    assert rel(dw.t[:, :T], dw_ref[:, :T]) < DOT_TOL and rel(dw.t[:, T], dw_ref[:, T]) < DOT_TOL


def test_attn_values_bwd_with_a_weight_table_off_16_byte_alignment():
    """T = 16, wdim = 32 with wmv 4 bytes off 16-byte alignment: the 16-byte weight loads of the fast form would be misaligned.
    include/mgf.h documents no alignment for mgf_attn_bwd_job.wmv and no refusal, so the entry must take its generic loop and compute."""
    _lib, L = _lib_()
    T, cs = 16, (64, 20)
    n, D = lc.LATENT_N, lc.LATENT_WDIM
    inp = lc.latent_side_inputs(T, cs)
    _vwb, dyc_ref, _dwg, _dw = lc.latent_side_ref(inp, 1.0)
    wmv = [Guarded((c, D), w, offset=1) for c, w in zip(cs, inp["wmv"])]
    assert all(w.ptr() % 16 == 4 for w in wmv)
    dvwb = [g_in(d) for d in inp["dvwb"]]
    atable = _device_table([_lib.AttnBwdJob(wmv[j].ptr(), dvwb[j].ptr(), cs[j], 0) for j in range(2)], _lib.AttnBwdJob)
    dyc = g_out(n, 2, T, D)
    _lib.check(L.mgf_attn_values_bwd_multi(dyc.ptr(), atable.data_ptr(), 2, n, T, D, _lib.stream_ptr()))
    assert dyc.written() and dyc.guard_intact()
    assert rel(dyc.t, dyc_ref) < DOT_TOL
    # against the aligned call (the fast form): the same sums in another order
    al = [g_in(w) for w in inp["wmv"]]
    atable2 = _device_table([_lib.AttnBwdJob(al[j].ptr(), dvwb[j].ptr(), cs[j], 0) for j in range(2)], _lib.AttnBwdJob)
    dyc2 = g_out(n, 2, T, D)
    _lib.check(L.mgf_attn_values_bwd_multi(dyc2.ptr(), atable2.data_ptr(), 2, n, T, D, _lib.stream_ptr()))
    assert rel(dyc2.t, dyc_ref) < DOT_TOL and rel(dyc2.t, dyc.t) < DOT_TOL


# ================================================================================================ 2. whole generators
@functools.lru_cache(maxsize=None)
def _generator(cid):
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import make_state_dict
    cfg = lc.generator_cases()[cid]
    sd = make_state_dict(cfg, seed=lc.weights_seed(cid))
    return Generator(sd, cfg, "cuda", max_batch=3), sd, cfg


@functools.lru_cache(maxsize=None)
def _oracle(cid):
    G, sd, cfg = _generator(cid)
    return lc.oracle_image_and_maps(cid, cfg, sd)            # shared by the tests below, never modified


@pytest.mark.parametrize("cid", lc.GENERATOR_IDS)
def test_generator_image_and_assignments_at_other_latent_counts(cid):
    from oracle.generator_ref import generator_ref, to_torch_state
    G, sd, cfg = _generator(cid)
    T, R = cfg.k - 1, cfg.img_resolution
    z, ref, maps = _oracle(cid)
    img, att = G(z.cuda(), None, noise_mode="const", return_att=True, att_format="maps")
    assert tuple(img.shape) == (3, 3, R, R)
    assert rel(img, ref) < PIX_TOL
    assert sorted(att) == sorted(maps) and len(maps) >= 5
    for key, want in maps.items():
        probs, argmax = att[key]
        assert tuple(probs.shape) == tuple(want.shape) and probs.shape[-1] == T and tuple(argmax.shape) == tuple(want.shape[:2]), key
        assert float((probs.cpu() - want).abs().max()) < 1e-4, key
        dec = lc.decided(want)
        assert 1.0 - float(dec.double().mean()) <= lc.MAX_UNDECIDED, key
        am = argmax.cpu().long()
        assert int(am.min()) >= 0 and int(am.max()) < T, key
        assert bool((am[dec] == want.argmax(-1)[dec]).all()), key
        if T == 1:
            assert bool((am == 0).all()), key
    ref0 = generator_ref(to_torch_state(sd), z[:2], cfg, "none", truncation_psi=0.6)
    img0 = G(z[:2].cuda(), None, noise_mode="none", truncation_psi=0.6)[0]
    assert tuple(img0.shape) == (2, 3, R, R)
    assert rel(img0, ref0) < PIX_TOL


@pytest.mark.parametrize("cid", lc.GENERATOR_IDS)
def test_attention_tensor_at_other_latent_counts(cid):
    """return_att=True in the reference's format: [n, k-1, layers, 1, R, R], each layer's probabilities replicated nearest-neighbour
    (mgf_att_map_upsample_f32 with t = k - 1), a distribution over the latent axis at every pixel."""
    G, sd, cfg = _generator(cid)
    T, R = cfg.k - 1, cfg.img_resolution
    z, ref, maps = _oracle(cid)
    zc = z.cuda()
    _img, att = G(zc, None, noise_mode="const", return_att=True, att_format="maps")
    att = {k: (p.clone(), a.clone()) for k, (p, a) in att.items()}
    img, t = G(zc, None, noise_mode="const", return_att=True, att_format="tensor")
    names = [lp.name for lp in G.plan.layers if lp.name in att]
    assert tuple(t.shape) == (3, T, len(names), 1, R, R) and len(names) == len(maps)
    for i, name in enumerate(names):
        probs = att[name][0]
        r = int(round(probs.shape[1] ** 0.5))
        want = probs.reshape(3, r, r, T).permute(0, 3, 1, 2).repeat_interleave(R // r, dim=2).repeat_interleave(R // r, dim=3)
        assert torch.equal(t[:, :, i, 0], want), name
    assert torch.equal(G.list2tensor(att), t)
    assert float((t.double().sum(1) - 1).abs().max()) < 1e-5
    assert rel(img, ref) < PIX_TOL


@pytest.mark.parametrize("cid", lc.GENERATOR_IDS)
def test_generator_gradient_at_other_latent_counts(cid):
    """GeneratorGrad.forward / backward: dz against autograd through the CPU oracle."""
    from morphganformer_amd.grad import GeneratorGrad
    from oracle.generator_ref import generator_ref, to_torch_state
    G, sd, cfg = _generator(cid)
    gg = GeneratorGrad(G)
    z, target = lc.gradient_inputs(cid, cfg)
    z = z.requires_grad_(True)
    img_ref = generator_ref(to_torch_state(sd), z, cfg, "const")
    (dz_ref,) = torch.autograd.grad((img_ref - target).square().mean(dim=(1, 2, 3)).sum(), z)
    img = gg.forward(z.detach().cuda(), noise_mode="const")
    assert rel(img, img_ref) < PIX_TOL
    dz = gg.backward(2.0 * (img - target.cuda()) / target[0].numel())
    assert tuple(dz.shape) == (2, cfg.k, cfg.z_dim)
    assert rel(dz, dz_ref) < GRAD_TOL
    assert gg.attn_defer is None                                     # below 16 latents the by-products keep their per-layer launches


@pytest.mark.parametrize("cid", lc.WPLUS_IDS)
def test_wplus_gradient_at_other_latent_counts(cid):
    """Per-layer latents ws [n, k, num_ws, D]: d mean(img^2) / d ws by GeneratorGrad.backward_ws against autograd through the oracle's
    synthesis network; the gates of test_wplus_gradient_matches_reference_module (overall, per layer slot, and summed over the slots)."""
    from morphganformer_amd.grad import GeneratorGrad
    from oracle.generator_ref import mapping_ref, synthesis_ref, to_torch_state
    G, sd, cfg = _generator(cid)
    tsd = to_torch_state(sd)
    gg = GeneratorGrad(G)
    torch.manual_seed(800 + cfg.k)
    w = mapping_ref(tsd, torch.randn(2, cfg.k, cfg.z_dim), cfg).detach()
    ws = (w[:, :, None] + 0.3 * float(w.std()) * torch.randn(2, cfg.k, cfg.num_ws, cfg.w_dim)).requires_grad_(True)
    img_ref = synthesis_ref(tsd, ws, cfg, "const")
    (dws_ref,) = torch.autograd.grad(img_ref.square().mean(), ws)
    img = gg.forward(ws=ws.detach().cuda(), noise_mode="const")
    assert rel(img, img_ref) < PIX_TOL
    dimg = 2.0 * img / img.numel()
    dws = gg.backward_ws(dimg).clone()
    assert tuple(dws.shape) == (2, cfg.k, cfg.num_ws, cfg.w_dim)
    assert rel(dws, dws_ref) < GRAD_TOL
    for s in range(cfg.num_ws):
        assert rel(dws[:, :, s], dws_ref[:, :, s]) < 5 * GRAD_TOL, s
    assert rel(gg.backward_w(dimg), dws_ref.sum(dim=2)) < GRAD_TOL


def test_gradient_projection_at_k_9_matches_autograd_adam():
    """Three steps of the gradient-mode loop at k = 9 (LPIPS squeeze + MSE, hipGraph replay) against torch autograd + torch.optim.Adam
    through the CPU oracle: noise, Adam and the best-of bookkeeping over k * w_dim = 288 numbers instead of 544; the tolerances of
    test_gradient_projection_matches_autograd_adam."""
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.lpips import PerceptualLoss
    from morphganformer_amd.projection import GradientProjectionEngine
    pr = lc.projection_reference()
    cfg, args, ref, steps, latent_mean = pr["cfg"], pr["args"], pr["ref"], pr["steps"], pr["latent_mean"]
    G = Generator(pr["sd"], cfg, "cuda", max_batch=1)
    pl = PerceptualLoss(net="squeeze", allow_random_backbone=True)
    eng = GradientProjectionEngine(G, pr["target"].cuda(), latent_mean.cuda(), 1.0, args, percept=pl, eps=pr["eps"].cuda(),
                                   noise_mode="const", use_graph=True)
    traj = []
    for i in range(steps):
        eng.run(1)
        traj.append(eng.latent_in.cpu().clone())
    lat, bstep, bloss, losses = eng.result()
    assert tuple(lat.shape)[-2:] == (cfg.k, cfg.z_dim)
    moved = float((ref[4][-1] - latent_mean).abs().max())
    assert moved > 5 * args.lr * 0.2, "the oracle run must actually move the latent"
    for i in range(steps):
        assert float((traj[i] - ref[4][i]).abs().max()) < 0.05 * args.lr * (i + 1), i
    got, want = np.asarray(losses, np.float64), np.array(ref[3])
    assert got.shape == want.shape and not np.isnan(got).any()
    assert np.abs(got - want).max() < 1e-3 * np.abs(want).max()
    assert bstep == ref[1]
    assert float((lat.cpu() - ref[0]).abs().max()) < 0.05 * args.lr * steps


@pytest.mark.parametrize("bad,names", [(dict(k=18), "16"), (dict(w_dim=64, z_dim=64), "32")])
def test_generator_refuses_unsupported_latent_counts_and_widths_at_construction(bad, names):
    """17 local latents / a latent width of 64: refused by Generator.__init__ with the limit in the message, before a weight is uploaded,
    a kernel launched or a workspace sized -- no device memory is taken and no half-built Generator stays behind."""
    import dataclasses
    import gc
    from morphganformer_amd import _lib
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import GeneratorConfig, make_state_dict
    cfg = dataclasses.replace(GeneratorConfig(img_resolution=32, channel_base=256, channel_max=16), **bad)
    sd = make_state_dict(cfg, seed=1)
    torch.cuda.synchronize()
    gc.collect()
    before = torch.cuda.memory_allocated()
    # (a Generator whose constructor did not finish: the workspace fields are the last it sets)
    half_built = lambda: [o for o in gc.get_objects() if type(o) is Generator and not hasattr(o, "n_attn_jobs")]
    with pytest.raises((_lib.MgfError, ValueError), match=names) as ei:
        Generator(sd, cfg, "cuda", max_batch=1)
    assert str(ei.value).startswith("Generator:")                    # the constructor's own check, not a C entry's refusal mid-forward
    del ei
    gc.collect()
    assert torch.cuda.memory_allocated() == before
    assert half_built() == []
