"""Workload of tools/record_calls.py behind profiles/projection_modes_ab.jsonl: every launch mode of both projection engines on the tiny
64^2 generator.  A configuration records the whole life of an engine -- construction, capture-free run, retarget / rewind -- under the
Recorder (eager), then lives the same life under graph replay; both hash best_latent, best_step, min_loss, losses and, where they exist,
the improvement trail, best_noises and id_trace.

    python tools/record_calls.py tools/projection_modes_ab.py --run head --out profiles/projection_modes_ab.jsonl
"""
import contextlib
import hashlib
import warnings

import numpy as np
import torch

DEV = "cuda"
STEPS = 14


def sha(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()[:16]


def hashes(eng, tag=""):
    torch.cuda.synchronize()
    res = {f: sha(getattr(eng, f)) for f in ("best_latent", "best_step", "min_loss", "losses")}
    if eng.keep_images > 0:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            trail = eng.improvements()
        res["trail"] = sha(np.array([[s, l] for s, l, _ in trail], dtype=np.float64))
        res["trail_images"] = sha(torch.stack([img.cpu() for _, _, img in trail])) if trail else "none"
    if getattr(eng, "best_noises", None):
        res["best_noises"] = sha(torch.cat([v.reshape(-1) for v in eng.best_noises.values()]))
        res["noises"] = sha(torch.cat([v.reshape(-1) for v in eng.noises.values()]))
    if getattr(eng, "id_trace", None) is not None:
        res["id_trace"] = sha(eng.id_trace)
    if hasattr(eng, "gen_ctr"):
        res["gen_ctr"] = sha(eng.gen_ctr)
    return {k + tag: v for k, v in res.items()}


def host_detector(lm_t, float_input):
    """A detector that reads what it is handed: landmarks shifted by a statistic of the image, "no face" on every fifth value of it."""
    def detect(img):
        m = int(np.abs(img).sum() * 8) if float_input else int(img.astype(np.int64).sum())
        return None if m % 5 == 0 else lm_t + (m % 7)
    return detect


def device_detector(lm_t):
    base = torch.as_tensor(lm_t, device=DEV)

    def model(img):
        pooled = torch.nn.functional.adaptive_avg_pool2d(img[:, :1], (68, 2)).reshape(img.shape[0], 68, 2).double()
        return base[None] + torch.round(60 * pooled), (img.mean(dim=(1, 2, 3)) > -10).to(torch.int32)
    return model


def config(name, gradient=False, runs=(STEPS,), second=None, percept=True, terms=(), detector=None, targets=1, pair=False, **extra):
    """runs: the run() calls of the first life (None = all that is left).  second: "retarget" or "rewind", then the same runs again.
    terms: "bio", "mdf", "region", "lbp".  Everything else goes to the engine (args_* to ProjectionArgs)."""
    def run(Recorder):
        from morphganformer_amd import lbp
        from morphganformer_amd.engine import Generator
        from morphganformer_amd.iresnet import BiometricLoss, IResNetEmbedder
        from morphganformer_amd.lpips import PerceptualLoss
        from morphganformer_amd.mdf import MDFLoss, random_discriminators
        from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, ProjectionEngine, synthetic_landmarks
        from morphganformer_amd.synth_weights import TINY, make_state_dict, synthetic_latents
        res = TINY.img_resolution
        kw = dict(extra)
        akw = {k[5:]: kw.pop(k) for k in list(kw) if k.startswith("args_")}
        batch = kw.get("batch", 1)
        G = Generator(make_state_dict(TINY, seed=0), TINY, DEV, max_batch=max(batch, targets))
        z = torch.from_numpy(synthetic_latents(TINY, targets + 2, seed=11)).to(DEV)
        tg = torch.cat([G(z[j:j + 1], None, noise_mode="const")[0].clamp(-1, 1) for j in range(targets + 2)]).contiguous()
        pool = akw.get("pool_above", 0)
        if pool:
            f = res // pool
            tg = tg.reshape(-1, 3, pool, f, pool, f).mean(dim=(3, 5)).contiguous()
        lms = [synthetic_landmarks(STEPS, res, seed=40 + j) for j in range(targets + 2)]
        kw.setdefault("noise_mode", "const")
        kw.update(use_mse=True, seed=9)
        if "lbp" in terms:
            u8 = lambda t: ((t[0].permute(1, 2, 0) * 127.5 + 127.5).round().clamp(0, 255).to(torch.uint8)).cpu().numpy()
            akw.update(pixel_term="lbp", min_loss_init=1.0)
        elif targets == 1:
            kw.update(lm_target=lms[0][0])
            if detector is None:
                kw.update(lm_steps=lms[0][1])
        else:
            kw.update(lm_target=np.stack([l[0] for l in lms[:targets]]), lm_steps=np.stack([l[1] for l in lms[:targets]]))
        if detector == "model":
            kw.update(landmark_model=device_detector(lms[0][0]))
        elif detector is not None:
            kw.update(landmark_fn=host_detector(lms[0][0], detector == "float"), landmark_input=detector)
        if pair:
            kw.update(target_b=tg[targets:2 * targets] if targets > 1 else tg[1:2], morph_alpha=0.3)
        if "region" in terms:
            side = pool or res
            kw.update(region_weight=torch.rand(side, side, generator=torch.Generator().manual_seed(5)) + 0.05)
        args = ProjectionArgs(step=STEPS, lr=0.05, lr_rampup=0.2, noise_regularize=1.0, **akw)
        out = {}
        for mode in ("eager", "graph"):
            torch.manual_seed(3)                                     # keys the generator's per-layer noise stream (noise_mode="random")
            with (Recorder() if mode == "eager" else contextlib.nullcontext()) as rec:
                if "lbp" in terms:
                    kw.update(lbp_target=lbp.target_feature(u8(tg[:1])))
                if "bio" in terms:
                    kw.update(biometric=BiometricLoss(IResNetEmbedder(None, depth=18, n=max(batch, targets), device=DEV)), gamma=1e-3)
                if "mdf" in terms:
                    kw.update(mdf=MDFLoss(random_discriminators(2), differentiable=gradient))
                if percept and "lbp" not in terms:
                    kw.update(percept=PerceptualLoss(net="squeeze", allow_random_backbone=True))
                cls = GradientProjectionEngine if gradient else ProjectionEngine
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")                  # keep_images < batch warns: that is the configuration
                    eng = cls(G, tg[:targets], z[-1], 1.0, args, use_graph=mode == "graph", **kw)
                eng.graph_debug = not (eng.pipeline or eng.callback_graphs)      # (the plain graph's kernel nodes are counted below)
                for n in runs:
                    eng.run(n)
                r = hashes(eng)
                if second == "retarget":
                    rkw = dict(lm_target=lms[1][0]) if "lm_target" in kw else {}
                    if "lm_steps" in kw:
                        rkw.update(lm_steps=lms[1][1])
                    if "lbp" in terms:
                        rkw.update(lbp_target=lbp.target_feature(u8(tg[1:2])))
                    eng.retarget(tg[1:2], seed=10, **rkw)
                elif second == "rewind":
                    eng.rewind()
                if second:
                    for n in runs:
                        eng.run(n)
                    r.update(hashes(eng, "/second"))
            out[mode] = r
            if mode == "eager":
                out["recorder"] = rec
            elif getattr(eng, "graph", None) is not None:
                from tools.lpips_refactor_ab import kernel_nodes
                out["graph_kernel_nodes"] = kernel_nodes(eng.graph)
            del eng
        return out
    return name, run


def configs():
    lit = lambda name, **kw: config("lit/" + name, **{"batch": 4, **kw})
    grad = lambda name, **kw: config("grad/" + name, gradient=True, **kw)
    two = (6, None)                                                # two run() calls; at batch 4 over 14 steps: 2 + 2 launch sequences
    return [
        lit("batch1", batch=1), lit("batch4_ragged"), lit("random_noise", noise_mode="random"),
        lit("pipeline_odd_sequences", pipeline=True, runs=(4, 8)),               # 1 + 2 = 3 launch sequences, the run stops before the end
        lit("pipeline_to_the_end", pipeline=True, runs=two),
        lit("trail_spills", keep_images=4, runs=two), lit("trail_pipelined", keep_images=4, pipeline=True, runs=two),
        lit("trail_smaller_than_batch", keep_images=2),
        lit("landmark_fn_float", detector="float", runs=two), lit("landmark_fn_gray_u8", detector="gray_u8", runs=two),
        lit("landmark_fn_gray_u8_trail", detector="gray_u8", keep_images=4), lit("landmark_model", detector="model"),
        lit("latent_copies", args_latent_copies=3), lit("pool_above", args_pool_above=32), lit("lbp", terms=("lbp",), percept=False),
        lit("region_weight", terms=("region",)), lit("biometric_mdf", terms=("bio", "mdf")),
        lit("plain/retarget", second="retarget"), lit("pipeline/retarget", pipeline=True, runs=(4, 8), second="retarget"),
        lit("gray_u8/retarget", detector="gray_u8", second="retarget"), lit("lbp/retarget", terms=("lbp",), percept=False, second="retarget"),
        lit("trail/retarget", keep_images=4, second="retarget"),
        grad("z"), grad("wplus", latent_space="w+"), grad("two_lockstep", targets=2), grad("pair", pair=True),
        grad("pair_biometric", pair=True, terms=("bio",), id_balance=0.5), grad("biometric", terms=("bio",)),
        grad("optimize_noise_randn", optimize_noise=True, noise_init="randn"), grad("optimize_noise_const", optimize_noise=True, noise_init="const"),
        grad("mdf", terms=("mdf",)), grad("landmark_fn_float", detector="float"), grad("region_weight", terms=("region",)),
        grad("z/rewind", second="rewind", runs=two), grad("optimize_noise/rewind", optimize_noise=True, second="rewind"),
        grad("z/retarget", second="retarget"),
    ]
