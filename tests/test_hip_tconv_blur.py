"""The fused up-sampling launch (csrc/tconv_blur.hip: mgf_tconv3x3s2_blur_f32 -- stride-2 transposed 3x3 conv + 4x4 blur + noise / bias /
leaky ReLU in one strip-walking kernel) against float64, against the three launches it replaces (conv.TCONV_BLUR = False is the same
switch as MGF_TCONV_BLUR=0), for batch invariance, and inside the generator and the literal projection loop.

Head-room of the float64 gate, max |got - ref64| / (r A), as measured on an MI355X: see profiles/tconv_blur_micro.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_replay import M_DIRECT, REL_BOUNDS  # noqa: E402

pytestmark = pytest.mark.gpu

F1331 = [1.0, 3.0, 3.0, 1.0]
CANARY = 12345.678
FUSED = "tconv_blur_kernel"
TAPLIST_TCONV = "conv_taps_kernel<1, 2, 1, true, 10, 0>"
ADOPTED_RES = (1024,)                 # blocks of the 1024^2 generator whose conv0 takes the fused launch (profiles/tconv_blur_micro.txt)


def pipeline(x, w, s, d, f1, noise, strength, bias, lrelu, gain, fir_gain=4.0):
    """The reference in x's dtype: conv_transpose2d(stride 2) on s x, times d, 4x4 FIR (true convolution, padding 1, gain 4), + noise *
    strength, + bias, leaky ReLU 0.2 (or linear), times gain."""
    F = torch.nn.functional
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    xs = x if s is None else x * s[:, :, None, None]
    t = F.conv_transpose2d(xs, w.transpose(0, 1), stride=2)
    if d is not None:
        t = t * d[:, :, None, None]
    f2 = torch.outer(f1, f1).flip(0, 1) * fir_gain
    y = F.conv2d(F.pad(t, (1, 1, 1, 1)).reshape(n * cout, 1, 2 * h + 3, 2 * wd + 3), f2[None, None]).reshape(n, cout, 2 * h, 2 * wd)
    if noise is not None:
        y = y + (noise * strength).reshape(-1, 1, 2 * h, 2 * wd)
    if bias is not None:
        y = y + bias[None, :, None, None]
    if lrelu:
        y = F.leaky_relu(y, 0.2)
    return y * gain


def make_case(n, cin, cout, h, w, seed, per_sample_noise, with_in_scale, taps):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    c = {"x": rn(n, cin, h, w), "w": rn(cout, cin, 3, 3) / math.sqrt(9 * cin),
         "s": 1 + 0.2 * rn(n, cin) if with_in_scale else None, "d": 1 + 0.2 * rn(n, cout),
         "f1": torch.tensor(taps) / sum(taps), "noise": rn(n if per_sample_noise else 1, 4 * h * w), "strength": torch.tensor(0.7),
         "bias": 0.3 * rn(cout)}
    return c


def fused_launch(c, lrelu, gain, out=None):
    """The kernel itself (no predicate, no fall-back): -> y [n, cout, 2h, 2w]."""
    from morphganformer_amd import _lib
    from morphganformer_amd import conv as cv
    import ctypes as C
    dv = {k: (None if v is None else v.cuda().contiguous()) for k, v in c.items()}
    n, cin, h, w = c["x"].shape
    pc = cv.pack_weights(dv["w"])
    if out is None:
        out = torch.empty(n, pc.cout, 2 * h, 2 * w, device="cuda")
    ep = _lib.make_epilogue(bias=dv["bias"], noise=dv["noise"], noise_strength=dv["strength"], noise_n=dv["noise"].shape[0],
                            act="lrelu" if lrelu else "linear", alpha=0.2, gain=gain)
    sy = out.stride()
    rc = _lib.lib().mgf_tconv3x3s2_blur_f32(out.data_ptr(), dv["x"].data_ptr(), pc.wp.data_ptr(), _lib.ptr(dv["s"]), _lib.ptr(dv["d"]),
                                            dv["f1"].data_ptr(), 4.0, n, cin, h, w, pc.cout, pc.cout_pad, sy[2], sy[1], sy[0],
                                            0 if dv["d"] is None else dv["d"].stride(0), C.byref(ep), _lib.stream_ptr())
    _lib.check(rc, "tconv3x3s2_blur")
    torch.cuda.synchronize()
    return out


def three_launches(c, lrelu, gain):
    """Today's path called by hand: tap-list transposed conv (+ border) into t, then the blur with the epilogue."""
    from morphganformer_amd import _lib
    from morphganformer_amd import conv as cv
    dv = {k: (None if v is None else v.cuda().contiguous()) for k, v in c.items()}
    n, cin, h, w = c["x"].shape
    pc = cv.pack_weights(dv["w"])
    ep = _lib.make_epilogue(bias=dv["bias"], noise=dv["noise"], noise_strength=dv["strength"], noise_n=dv["noise"].shape[0],
                            act="lrelu" if lrelu else "linear", alpha=0.2, gain=gain)
    t = cv.tconv3x3s2_forward(dv["x"], pc, in_scale=dv["s"], out_scale=dv["d"])
    y = torch.empty(n, pc.cout, 2 * h, 2 * w, device="cuda")
    cv.upfirdn_into(y, t, torch.outer(dv["f1"], dv["f1"]).contiguous(), up=1, pad=(1, 1, 1, 1), gain=4.0, epilogue=ep, separable=True)
    torch.cuda.synchronize()
    return y


# (n, cin, cout, h, w, per-sample noise, in_scale, leaky ReLU, filter taps): the smallest shapes that reach each path of the walk --
# smaller than every tile; two strips (30 + 7), a ragged last row step, two channel tiles, two K chunks, an asymmetric filter (the
# orientation of the convolution); three strips (30 + 30 + 4), a one-row tail (34 output rows = 2 steps + 2 rows), shared noise, linear
CASES = [(1, 8, 32, 4, 4, True, True, True, F1331),
         (2, 16, 64, 11, 37, True, True, True, [1.0, 3.0, 4.0, 2.0]),
         (3, 64, 32, 17, 64, False, False, False, F1331)]


@pytest.mark.parametrize("n,cin,cout,h,w,psn,ins,lrelu,taps", CASES)
def test_kernel_against_float64(n, cin, cout, h, w, psn, ins, lrelu, taps):
    """Per element |got - ref64| <= c A with tests/conv_replay.py's rule for kernels that differ from the float32 direct form in summation
    order only (m = 4): c = max(4 r, sqrt(K) 2^-24), r = max |ref32 - ref64| / A, K = 36 cin, A = the pipeline on absolute values; and
    max-norm relative error <= REL_BOUNDS["tconv3x3s2_forward"].  The output sits between two canary bands."""
    c = make_case(n, cin, cout, h, w, 1000 + h * 7 + w, psn, ins, taps)
    gain = math.sqrt(2.0)
    f64 = lambda v: None if v is None else v.double()
    ab = lambda v: None if v is None else v.double().abs()
    ref64 = pipeline(*[f64(c[k]) for k in ("x", "w", "s", "d", "f1", "noise", "strength", "bias")], lrelu, gain)
    ref32 = pipeline(*[c[k] for k in ("x", "w", "s", "d", "f1", "noise", "strength", "bias")], lrelu, gain).double()
    A = pipeline(*[ab(c[k]) for k in ("x", "w", "s", "d", "f1", "noise", "strength", "bias")], lrelu, gain)
    numel, band = n * cout * 4 * h * w, 4096
    buf = torch.full((numel + 2 * band,), CANARY, device="cuda")
    out = buf[band:band + numel].view(n, cout, 2 * h, 2 * w)
    got = fused_launch(c, lrelu, gain, out=out).double().cpu()
    assert bool((buf[:band] == CANARY).all()) and bool((buf[band + numel:] == CANARY).all()), "write outside the output"
    r = float(((ref32 - ref64).abs() / A).max())
    cc = max(M_DIRECT * r, math.sqrt(36 * cin) * 2.0 ** -24)
    err = (got - ref64).abs()
    rel = float(err.max() / ref64.abs().max())
    print(f"tconv_blur n={n} cin={cin} cout={cout} {h}x{w}: r={r:.3e} c={cc:.3e} head-room max|got-ref64|/(r A)={float((err / (r * A)).max()):.3f} "
          f"max|got-ref64|/(c A)={float((err / (cc * A)).max()):.3f} max-norm rel={rel:.3e}")
    assert not torch.isnan(got).any()
    assert bool((err <= cc * A).all()), float((err / (cc * A)).max())
    assert rel <= REL_BOUNDS["tconv3x3s2_forward"]


def test_batch_invariance():
    """The batch launch equals four single-sample launches bit for bit (the literal loop's "same result as the sequential loop")."""
    n = 4
    c = make_case(n, 16, 64, 11, 37, 77, True, True, F1331)
    whole = fused_launch(c, True, math.sqrt(2.0))
    for j in range(n):
        one = {k: (v[j:j + 1] if k in ("x", "s", "d", "noise") else v) for k, v in c.items()}
        assert torch.equal(fused_launch(one, True, math.sqrt(2.0))[0], whole[j]), j


@pytest.mark.parametrize("cin,cout,h", [(128, 64, 256), (64, 32, 512)])
def test_fused_vs_three_launches_at_engine_shapes(cin, cout, h):
    c = make_case(1, cin, cout, h, h, cin + h, True, True, F1331)
    new = fused_launch(c, True, math.sqrt(2.0))
    old = three_launches(c, True, math.sqrt(2.0))
    assert float((new - old).abs().max()) <= 2e-5 * float(old.abs().max())


def test_wrapper_falls_back_bit_for_bit(monkeypatch):
    """A shape the predicate refuses (cin % 8 != 0) goes through the wrapper to exactly the three launches; one it accepts runs the kernel."""
    from morphganformer_amd import _lib
    from morphganformer_amd import conv as cv
    monkeypatch.setattr(cv, "TCONV_BLUR_MIN_WGS", 0)
    for cin, fused in ((12, False), (16, True)):
        c = make_case(2, cin, 32, 9, 13, 5 + cin, True, True, [1.0, 3.0, 4.0, 2.0])
        dv = {k: v.cuda().contiguous() for k, v in c.items()}
        pc = cv.pack_weights(dv["w"])
        ep = _lib.make_epilogue(bias=dv["bias"], noise=dv["noise"], noise_strength=dv["strength"], noise_n=2, act="lrelu", alpha=0.2, gain=1.5)
        out = torch.empty(2, 32, 18, 26, device="cuda")
        assert cv.tconv_blur_ok(2, cin, 9, 13, 32, out, dv["f1"], ep) == fused
        cv.profile_begin()
        y = cv.tconv3x3s2_blur_forward(dv["x"], pc, dv["f1"], 4.0, in_scale=dv["s"], out_scale=dv["d"], epilogue=ep, out=out)
        names = [r[0] for r in cv.profile_end()]
        assert (FUSED in names) == fused, names
        ref = three_launches(c, True, 1.5)
        if fused:
            assert float((y - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
            monkeypatch.setattr(cv, "TCONV_BLUR", False)          # the switch, read at call time
            assert torch.equal(cv.tconv3x3s2_blur_forward(dv["x"], pc, dv["f1"], 4.0, in_scale=dv["s"], out_scale=dv["d"], epilogue=ep), ref)
        else:
            assert torch.equal(y, ref)


def _no_attention_tiny():
    """TINY's size with 32 channels up to 64^2 and attention only below 16^2: its 16^2 .. 64^2 blocks have the up-sampling layers the fused
    launch serves (TINY itself has attention, 16 or 8 channels, on all of them, and keeps the three launches whatever the switch says)."""
    from morphganformer_amd.synth_weights import GeneratorConfig
    return GeneratorConfig(img_resolution=64, channel_base=2048, channel_max=32, attn_max_log2res=4)


def _profiled_forward(G, z):
    from morphganformer_amd import conv as cv
    cv.profile_begin()
    img = G.forward_workspace(z, None, noise_mode="const")[0].clone()
    return img, [r[0] for r in cv.profile_end()]


@pytest.mark.parametrize("which", ["tiny", "tiny_no_attention", "full1024"])
def test_generator_switch_on_equals_off(which, monkeypatch):
    from morphganformer_amd import conv as cv
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.synth_weights import FULL1024, TINY, make_state_dict, synthetic_latents
    cfg = {"tiny": TINY, "tiny_no_attention": _no_attention_tiny(), "full1024": FULL1024}[which]
    if which != "full1024":
        monkeypatch.setattr(cv, "TCONV_BLUR_MIN_WGS", 0)         # (FULL1024 runs with the defaults)
    G = Generator(make_state_dict(cfg, seed=0), cfg, "cuda", max_batch=1)
    z = torch.from_numpy(synthetic_latents(cfg, 1, seed=77)).cuda()
    new, names_on = _profiled_forward(G, z)
    monkeypatch.setattr(cv, "TCONV_BLUR", False)
    old, names_off = _profiled_forward(G, z)
    assert FUSED not in names_off
    assert float((new - old).abs().max()) <= 1e-5 * float(old.abs().max())
    want = {"tiny": 0, "tiny_no_attention": 3, "full1024": len(ADOPTED_RES)}[which]
    assert names_on.count(FUSED) == want, names_on
    # ... and no tap-list transposed conv (nor its border launch's FIR partner) for those layers
    tl = lambda names: sum(1 for k in names if k.startswith("conv_taps_kernel<1, 2, 1,") or k.startswith("conv_taps_kernel<1, 1, 1,"))
    assert tl(names_off) - tl(names_on) == want, (names_on, names_off)


def test_literal_loop_graph_equals_eager_and_switch_off(monkeypatch):
    """Literal projection loop on the small generator with the path forced: graph replay == eager bit for bit; against the three launches
    the best step is equal and the loss history within 1e-5 relative."""
    from morphganformer_amd import conv as cv
    from morphganformer_amd.engine import Generator
    from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine, synthetic_landmarks
    from morphganformer_amd.synth_weights import make_state_dict, synthetic_latents
    cfg = _no_attention_tiny()
    monkeypatch.setattr(cv, "TCONV_BLUR_MIN_WGS", 0)
    G = Generator(make_state_dict(cfg, seed=0), cfg, "cuda", max_batch=1)
    steps = 8
    rng = np.random.Generator(np.random.PCG64(3))
    latent_mean = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32) * 0.1).cuda()
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32)).cuda()
    target = G(torch.from_numpy(synthetic_latents(cfg, 1, 1001)).cuda(), None, noise_mode="const")[0].clamp(-1, 1).clone()
    lm_t, lm_s = synthetic_landmarks(steps, 64, 9)

    def run(use_graph):
        eng = ProjectionEngine(G, target, latent_mean, 23.3, ProjectionArgs(step=steps), percept=None, lm_target=lm_t, lm_steps=lm_s,
                               eps=eps, noise_mode="const", use_graph=use_graph)
        return eng.run().result()
    cv.profile_begin()
    lat_e, step_e, loss_e, hist_e = run(False)
    assert FUSED in [r[0] for r in cv.profile_end()]
    lat_g, step_g, loss_g, hist_g = run(True)
    assert step_g == step_e and torch.equal(lat_g, lat_e) and np.array_equal(np.asarray(hist_g), np.asarray(hist_e))
    monkeypatch.setattr(cv, "TCONV_BLUR", False)
    lat_o, step_o, loss_o, hist_o = run(True)
    assert step_o == step_g
    assert np.abs(np.asarray(hist_g) - np.asarray(hist_o)).max() <= 1e-5 * np.abs(np.asarray(hist_o)).max()
