"""Cases, seeded inputs and float64 references shared by tests/test_hip_latent_counts.py (GPU) and tests/test_latent_counts_host.py (CPU):
the attention layers, the generator, its gradient and a projection at latent counts other than k = 17 (T = k - 1 local latents).

The float64 formulas are the ones tests/test_hip_ops.py::test_duplex_attention_forward_all_kernel_forms_vs_float64 and
tests/test_hip_gradient.py::test_duplex_attention_bwd_matches_autograd write out:
    S = x^T wqc + spos,  P = softmax(S),  y = x rsqrt(mean_c x^2 + 1e-8) (P vwb^T)  -> noise, bias, lrelu, gain, residual
with gradients from torch.autograd.grad on that float64 graph.  Nothing here is derived from a kernel.

"Exact where the top two are more than 1e-4 apart" leaves pixels out of the argmax comparisons.  How many is a CONDITION of the cases, not
a measurement: at most MAX_UNDECIDED (3 %, the figure of test_generator_random_configurations_vs_oracle) of a layer's pixels.  The host
test asserts it on the references alone for every case below, the GPU tests assert it again; a seed that misses it is replaced, never the cap.
"""
import math

import torch

MAX_UNDECIDED = 0.03
GAP = 1e-4
T_VALUES = (1, 2, 5, 8, 15)

# ---------------------------------------------------------------------------------------------- direct kernel cases
# (n, c, f): ragged channels + a ragged 16-pixel block / the register-resident kernel's shape at T = 16 / the MFMA kernel's shape at T = 16
_FWD_SHAPES = ((2, 20, 36), (3, 64, 80), (1, 256, 64))
# (n, c, f, T, with_epilogue): the epilogue runs in two shapes per T and is left out in one
FORWARD_CASES = [(n, c, f, T, (c != 64)) for T in T_VALUES for (n, c, f) in _FWD_SHAPES] + [(1, 512, 32, 8, True), (2, 20, 36, 16, True)]
# two more dispatch thresholds a real checkpoint with fewer latents crosses: 256 channels on a 64^2 map (the 4-blocks-per-workgroup kernel
# at T = 16) and a map of more than 16384 pixels (64-pixel blocks instead of 16-pixel ones; the last block ragged)
FORWARD_CASES += [(1, 256, 4096, 5, False), (1, 20, 16400, 5, True)]
# (n, c, res): ragged channels / a multiple of four / the MFMA shape at T = 16 / two staged tables above 64 KiB of LDS
_BWD_SHAPES = ((2, 20, 6), (2, 32, 8), (1, 256, 8), (1, 512, 4))
BACKWARD_CASES = [(n, c, res, T) for T in T_VALUES for (n, c, res) in _BWD_SHAPES]

EP_NOISE_STRENGTH, EP_ALPHA, EP_GAIN = 0.37, 0.2, 1.3


def attention_inputs(n, c, f, T, seed_base=0):
    """Seeded float64 operands of one attention launch."""
    torch.manual_seed(seed_base + 1000 * T + 7 * c + f)
    d = torch.float64
    return dict(x=torch.randn(n, c, f, dtype=d), wqc=torch.randn(c, T, dtype=d) / math.sqrt(c), spos=torch.randn(f, T, dtype=d),
                vwb=1 + 0.3 * torch.randn(n, c, T, dtype=d), noise=torch.randn(n, f, dtype=d), bias=torch.randn(c, dtype=d),
                res=torch.randn(n, c, f, dtype=d), da=torch.randn(n, c, f, dtype=d))


def attention_forward_ref(inp, with_ep):
    """-> scores S [n,f,T], probabilities P [n,f,T], output y [n,c,f], all float64."""
    x, vwb = inp["x"], inp["vwb"]
    S = torch.einsum("ncf,ct->nft", x, inp["wqc"]) + inp["spos"][None]
    P = torch.softmax(S, -1)
    r = torch.rsqrt(x.square().mean(1, keepdim=True) + 1e-8)
    y = x * r * torch.einsum("nft,nct->ncf", P, vwb)
    if with_ep:
        y = torch.nn.functional.leaky_relu(y + EP_NOISE_STRENGTH * inp["noise"][:, None] + inp["bias"][None, :, None], EP_ALPHA) * EP_GAIN + inp["res"]
    return S, P, y


def attention_backward_ref(inp):
    """-> P [n,f,T], dx [n,c,f], dvwb [n,c,T]: autograd of the layer without its epilogue, float64."""
    x = inp["x"].clone().requires_grad_(True)
    vwb = inp["vwb"].clone().requires_grad_(True)
    S = torch.einsum("ncf,ct->nft", x, inp["wqc"]) + inp["spos"][None]
    P = torch.softmax(S, -1)
    r = torch.rsqrt(x.square().mean(1, keepdim=True) + 1e-8)
    a = x * r * torch.einsum("nft,nct->ncf", P, vwb)
    dx, dv = torch.autograd.grad(a, (x, vwb), inp["da"])
    return P.detach(), dx, dv


def decided(values, gap=GAP):
    """[..., T] scores or probabilities -> bool [...]: the best entry leads the second best by more than `gap` (one latent: always)."""
    if values.shape[-1] < 2:
        return torch.ones(values.shape[:-1], dtype=torch.bool)
    top2 = torch.as_tensor(values).topk(2, -1).values
    return (top2[..., 0] - top2[..., 1]) > gap


def undecided_share(values, gap=GAP):
    return 1.0 - float(decided(values, gap).double().mean())


# ---------------------------------------------------------------------------------------------- latent-side reductions
LATENT_T = (1, 5, 16)
LATENT_CHANNELS = ((20, 20), (64, 64), (20, 64))        # channels of the two jobs of one launch
LATENT_WDIM, LATENT_N = 32, 2


def latent_side_inputs(T, cs, wdim=LATENT_WDIM, n=LATENT_N):
    """Two attention jobs (channels cs) and two style jobs (no demodulation: tests/style_demod_cases.py has the demodulated ones) of one
    latent-side launch, float64."""
    torch.manual_seed(500 + 10 * T + sum(cs))
    d = torch.float64
    k = T + 1
    out = dict(w=torch.randn(n, k, wdim, dtype=d), wmv=[torch.randn(c, wdim, dtype=d) / math.sqrt(wdim) for c in cs],
               bmv=[1 + torch.randn(c, dtype=d) for c in cs], dvwb=[torch.randn(n, c, T, dtype=d) for c in cs])
    style = []
    for cin, chunks in ((20, 3), (36, 17)):          # per-row sums over < 16 chunks by one lane and over >= 16 chunks by a wave
        style.append(dict(aff_w=torch.randn(cin, wdim, dtype=d), ds_part=torch.randn(n, cin, chunks, dtype=d), cin=cin, chunks=chunks,
                          aff_gain=1.0 / math.sqrt(wdim), style_gain=1.0 / math.sqrt(cin)))
    out["style"] = style
    return out


def latent_side_ref(inp, scale):
    """-> vwb per job [n,c,T], dyc [n,jobs,T,D], dwg [n,style jobs,D], dw [n,k,D]."""
    y = inp["w"][:, :-1]                                                                   # the local components
    vwb = [torch.einsum("ntj,cj->nct", y, wm) + b[None, :, None] for wm, b in zip(inp["wmv"], inp["bmv"])]
    dyc = torch.stack([torch.einsum("nct,ck->ntk", dv, wm) for dv, wm in zip(inp["dvwb"], inp["wmv"])], 1)
    dwg = torch.stack([s["aff_gain"] * s["style_gain"] * torch.einsum("ni,ik->nk", s["ds_part"].sum(-1), s["aff_w"]) for s in inp["style"]], 1)
    dw = torch.cat([dyc.sum(1), dwg.sum(1)[:, None]], 1) * scale
    return vwb, dyc, dwg, dw


# ---------------------------------------------------------------------------------------------- whole generators
def generator_cases():
    """{id: GeneratorConfig}: the 32^2 generator at k = 2, 6, 9, 16 and a 64^2 one (attention up to 32^2, TF-style mapping) at k = 9."""
    from morphganformer_amd.synth_weights import GeneratorConfig
    cases = {f"k{K}": GeneratorConfig(img_resolution=32, channel_base=256, channel_max=16, k=K) for K in (2, 6, 9, 16)}
    cases["k9_64"] = GeneratorConfig(img_resolution=64, channel_base=1024, channel_max=64, attn_max_log2res=6, normalize_global=False, k=9)
    return cases


GENERATOR_IDS = ("k2", "k6", "k9", "k16", "k9_64")
WPLUS_IDS = ("k6", "k16")
PROJECTION_ID = "k9_64"
PROJECTION_STEPS = 3


def weights_seed(cid):
    return 40 + GENERATOR_IDS.index(cid)


def image_latents(cid, cfg):
    """z [3, k, z_dim] of the image / attention tests (the first two rows also run with truncation_psi = 0.6 and no noise)."""
    torch.manual_seed(300 + GENERATOR_IDS.index(cid))
    return torch.randn(3, cfg.k, cfg.z_dim)


def gradient_inputs(cid, cfg):
    """z [2, k, z_dim] and the MSE target of the dz test."""
    torch.manual_seed(600 + GENERATOR_IDS.index(cid))
    z = torch.randn(2, cfg.k, cfg.z_dim)
    return z, torch.randn(2, 3, cfg.img_resolution, cfg.img_resolution) * 0.5


def projection_reference():
    """torch autograd + torch.optim.Adam through the CPU oracle at k = 9, MSE + LPIPS (squeeze), PROJECTION_STEPS steps: the operands and
    the run (oracle.loss_ref.projection_gradient_ref) that the engine's gradient-mode loop is compared with."""
    import os
    import numpy as np
    from morphganformer_amd.lpips import WEIGHTS_DIR
    from morphganformer_amd.projection import ProjectionArgs
    from morphganformer_amd.synth_weights import make_state_dict, synthetic_latents
    from oracle.generator_ref import generator_ref, to_torch_state
    from oracle.loss_ref import backbone_random, lpips_ref, mse_ref, projection_gradient_ref
    cid, steps = PROJECTION_ID, PROJECTION_STEPS
    cfg = generator_cases()[cid]
    sd = make_state_dict(cfg, seed=weights_seed(cid))
    tsd = to_torch_state(sd)
    rng = np.random.Generator(np.random.PCG64(9))
    latent_mean = torch.from_numpy(rng.standard_normal((cfg.k, cfg.z_dim)).astype(np.float32))
    eps = torch.from_numpy(rng.standard_normal((steps, 1, cfg.k, cfg.z_dim)).astype(np.float32))
    target = generator_ref(tsd, torch.from_numpy(synthetic_latents(cfg, 1, 1001)), cfg, "const").clamp(-1, 1)
    args = ProjectionArgs(step=steps, lr=0.05, lr_rampup=0.2)
    bb = backbone_random("squeeze", 0)
    lin = np.load(os.path.join(WEIGHTS_DIR, "lpips_lin_squeeze.npz"))
    lins = [torch.from_numpy(lin[f"lin{i}"]).float().reshape(-1) for i in range(7)]
    loss_fn = lambda i, img: lpips_ref(bb, lins, img, target).sum() + args.beta * mse_ref(img, target)
    ref = projection_gradient_ref(lambda z: generator_ref(tsd, z, cfg, "const"), loss_fn, latent_mean, 1.0, eps, steps, lr=args.lr,
                                  rampdown=args.lr_rampdown, rampup=args.lr_rampup)
    return dict(cfg=cfg, sd=sd, args=args, latent_mean=latent_mean, eps=eps, target=target, ref=ref, steps=steps)


def oracle_image_and_maps(cid, cfg, sd):
    """The CPU oracle on image_latents: -> z, image [3,3,R,R], {layer: probs [3,F,T]} (float32, the oracle's arithmetic)."""
    from oracle.generator_ref import generator_ref, to_torch_state
    z = image_latents(cid, cfg)
    taps = {}
    ref = generator_ref(to_torch_state(sd), z, cfg, "const", taps=taps)
    maps = {k[:-len(":probs")]: v.detach() for k, v in taps.items() if k.endswith(":probs")}
    return z, ref.detach(), maps
