"""Workload of tools/record_calls.py behind profiles/lpips_refactor_ab.jsonl: every public path of PerceptualLoss on small shapes
(stand-alone, spatial, the module call), the one stand-alone shape at which the merged Fire and the Winograd gradient launches engage
(600x520, one image), and both projection loops on the tiny 64^2 generator, eagerly (recorded) and under graph replay.

    python tools/record_calls.py tools/lpips_refactor_ab.py --run head --out profiles/lpips_refactor_ab.jsonl
"""
import contextlib
import ctypes
import hashlib

import numpy as np
import torch

from morphganformer_amd.lpips import PerceptualLoss

DEV = "cuda"


def sha(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()[:16]


def images(seed, *shape):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def probe(P, res, tag, x, per_tap=True):
    n = x.shape[0]
    out, d = torch.zeros(n, device=DEV), torch.ones_like(x)
    res[tag + "/distance"] = sha(P.distance_into(out, x))
    res[tag + "/distance_keep_taps"] = sha(P.distance_into(out, x, keep_taps=True))
    res[tag + "/grad_accumulated"] = sha(P.grad_into(d, scale=0.5, accumulate=True))
    res[tag + "/grad"] = sha(P.grad_into(d, scale=1.0))
    if per_tap:
        res[tag + "/per_tap"] = sha(P.distance_per_tap(x))


def alone(net, size, n):
    def run(Recorder):
        x, t, t2 = images(size + n, n, 3, size, size), images(size + n + 1, n, 3, size, size), images(size + n + 2, n, 3, size, size)
        weights = torch.rand(n, 1, size, size, generator=torch.Generator().manual_seed(size)) + 0.05
        res = {}
        with Recorder() as rec:
            P = PerceptualLoss(net=net, allow_random_backbone=True)
            for wtag, w in (("w_none", None), ("w_one", weights[:1]), ("w_n", weights), ("w_none_again", None)):
                P.set_region_weight(w)
                for ttag, tg in (("t_one", t[:1]), ("t_n", t)):
                    P.set_target(tg)
                    probe(P, res, f"{wtag}/{ttag}", x)
            for alpha in (0.0, 0.3, 1.0):
                P.set_target_pair(t, t2, alpha)
                res[f"pair{alpha}/offset"] = sha(P.pair_offset)
                probe(P, res, f"pair{alpha}", x, per_tap=False)
        return {"recorder": rec, "eager": res}
    return f"alone/{net}/n{n}/{size}x{size}", run


def spatial(net, n):
    def run(Recorder):
        x, t = images(7 + n, n, 3, 64, 64), images(8 + n, n, 3, 64, 64)
        res = {}
        with Recorder() as rec:
            P = PerceptualLoss(net=net, spatial=True, allow_random_backbone=True)
            P.set_target(t[:1])
            out = torch.empty(n, 1, 64, 64, device=DEV)
            taps = [torch.empty_like(out) for _ in P.lins]
            res["map"] = sha(P.distance_map_into(out, x, per_tap=taps))
            res["per_tap"] = sha(torch.stack(taps))
            val, layers = P(x, t, retPerLayer=True)
            res["call"], res["call_layers"] = sha(val), sha(torch.stack(layers))
        return {"recorder": rec, "eager": res}
    return f"spatial/{net}/n{n}/64x64", run


def module_call(weighted):
    def run(Recorder):
        x, t = images(21, 2, 3, 65, 65), images(22, 2, 3, 65, 65)
        with Recorder() as rec:
            P = PerceptualLoss(net="squeeze", allow_random_backbone=True)
            if weighted:
                P.set_region_weight(torch.rand(2, 1, 65, 65, generator=torch.Generator().manual_seed(3)) + 0.05)
            res = {"call": sha(P(x, t))}
        return {"recorder": rec, "eager": res}
    return f"call/squeeze/n2/{'n_weights' if weighted else 'unweighted'}", run


def merged():
    def run(Recorder):
        x, t = images(31, 1, 3, 600, 520), images(32, 1, 3, 600, 520)
        res = {}
        with Recorder() as rec:
            P = PerceptualLoss(net="squeeze", allow_random_backbone=True)
            P.set_target(t)
            probe(P, res, "t_one", x)
        return {"recorder": rec, "eager": res, "merged_fires": len(next(iter(P._feats.values())).merge)}
    return "alone/squeeze/n1/600x520", run


def kernel_nodes(graph):
    hip = ctypes.CDLL("libamdhip64.so")
    handle, n = ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(handle, nodes, ctypes.byref(n)) == 0
    kinds = []
    for node in nodes:
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(t)) == 0
        kinds.append(t.value)
    return kinds.count(0)                                        # hipGraphNodeTypeKernel


def loop(name, gradient, targets=1, pair=False, region=False, retarget=False):
    def run(Recorder):
        from morphganformer_amd.engine import Generator
        from morphganformer_amd.projection import GradientProjectionEngine, ProjectionArgs, ProjectionEngine, synthetic_landmarks
        from morphganformer_amd.synth_weights import TINY, make_state_dict, synthetic_latents
        steps = 6
        batch = 1 if gradient else 4
        G = Generator(make_state_dict(TINY, seed=0), TINY, DEV, max_batch=max(batch, targets))
        z = torch.from_numpy(synthetic_latents(TINY, targets + 2, seed=11)).to(DEV)
        tg = torch.cat([G(z[j:j + 1], None, noise_mode="const")[0].clamp(-1, 1) for j in range(targets + 2)]).contiguous()
        lms = [synthetic_landmarks(steps + 2, TINY.img_resolution, seed=40 + j) for j in range(targets + 2)]
        kw = dict(use_mse=True, noise_mode="const", seed=9)
        if targets == 1:
            kw.update(lm_target=lms[0][0], lm_steps=lms[0][1])
        else:
            kw.update(lm_target=np.stack([l[0] for l in lms[:targets]]), lm_steps=np.stack([l[1] for l in lms[:targets]]))
        if pair:
            kw.update(target_b=tg[1:2], morph_alpha=0.3)
        if region:
            kw.update(region_weight=torch.rand(64, 64, generator=torch.Generator().manual_seed(5)) + 0.05)
        out = {}
        for mode in ("eager", "graph"):
            P = PerceptualLoss(net="squeeze", allow_random_backbone=True)
            with (Recorder() if mode == "eager" else contextlib.nullcontext()) as rec:
                if gradient:
                    eng = GradientProjectionEngine(G, tg[:targets], z[-1], 1.0, ProjectionArgs(step=steps + 2), percept=P, use_graph=mode == "graph", **kw)
                else:
                    eng = ProjectionEngine(G, tg[:1], z[-1], 1.0, ProjectionArgs(step=steps + 2), percept=P, use_graph=mode == "graph", batch=batch, **kw)
                eng.graph_debug = True
                eng.run(steps)
                res = {"losses": sha(eng.losses), "best_latent": sha(eng.best_latent), "best_step": sha(eng.best_step)}
                if retarget:
                    eng.retarget(tg[1:2], lm_target=lms[1][0], lm_steps=lms[1][1], seed=10)
                    eng.run(steps)
                    res.update(losses2=sha(eng.losses), best_latent2=sha(eng.best_latent), best_step2=sha(eng.best_step))
            out[mode] = res
            if mode == "eager":
                out["recorder"] = rec
            elif gradient:
                out["graph_kernel_nodes"] = kernel_nodes(eng.graph)
            del eng
        return out
    return name, run


def configs():
    out = [alone(net, size, n) for net, size in (("squeeze", 65), ("squeeze", 128), ("vgg", 48), ("alex", 96)) for n in (1, 3)]
    out += [spatial(net, n) for net in ("squeeze", "vgg") for n in (1, 2)]
    out += [module_call(False), module_call(True), merged()]
    out += [loop("lit/batch4", False), loop("grad/one_target", True), loop("grad/two_lockstep", True, targets=2),
            loop("grad/pair", True, pair=True), loop("grad/region_weight", True, region=True), loop("lit/batch4/retarget", False, retarget=True)]
    return out
