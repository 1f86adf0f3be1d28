"""Workload of tools/record_calls.py for changes that must leave noise_mode="random" alone: the literal loop on the tiny generator with random
per-layer noise, plain and pipelined -- the eager run's C-ABI calls recorded, the eager and the replayed run's results hashed.

    python tools/record_calls.py tools/random_noise_calls_ab.py --run parentA --out FILE.jsonl      (the parent through MGF_PACKAGE_ROOT)
"""
import contextlib
import hashlib

import numpy as np
import torch

DEV = "cuda"


def sha(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()[:16]


def loop(name, pipeline):
    def run(Recorder):
        from morphganformer_amd.engine import Generator
        from morphganformer_amd.lpips import PerceptualLoss
        from morphganformer_amd.projection import ProjectionArgs, ProjectionEngine, synthetic_landmarks
        from morphganformer_amd.synth_weights import TINY, make_state_dict, synthetic_latents
        steps, batch = 22, 4
        G = Generator(make_state_dict(TINY, seed=0), TINY, DEV, max_batch=batch)
        z = torch.from_numpy(synthetic_latents(TINY, 2, seed=11)).to(DEV)
        tg = G(z[:1], None, noise_mode="const")[0].clamp(-1, 1).clone()
        lm = synthetic_landmarks(steps, TINY.img_resolution, seed=40)
        out = {}
        for mode in ("eager", "graph"):
            torch.manual_seed(77)
            P = PerceptualLoss(net="squeeze", allow_random_backbone=True)
            with (Recorder() if mode == "eager" else contextlib.nullcontext()) as rec:
                eng = ProjectionEngine(G, tg, z[1], 1.0, ProjectionArgs(step=steps), percept=P, use_mse=True, noise_mode="random", seed=9,
                                       lm_target=lm[0], lm_steps=lm[1], use_graph=mode == "graph", batch=batch, pipeline=pipeline, keep_images=4)
                eng.run()
                torch.cuda.synchronize()
                out[mode] = {"losses": sha(eng.losses), "best_latent": sha(eng.best_latent), "best_step": sha(eng.best_step),
                             "trail": [sha(im) for _, _, im in eng.improvements()]}
            if mode == "eager":
                out["recorder"] = rec
            del eng
        return out
    return name, run


def configs():
    return [loop("lit/random/plain", False), loop("lit/random/pipelined", True)]
