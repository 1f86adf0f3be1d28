"""Workload of tools/record_calls.py behind profiles/cli_drivers_ab.jsonl: every subcommand of the command line, driven in-process through
`cli.main(argv)` on the tiny 64^2 generator (a snapshot written by loader.save_snapshot_like_reference).  A configuration runs one command
under the Recorder and hashes every file the command wrote (SHA-256; a .mat past its 128-byte header, which holds the creation time).

    python tools/record_calls.py tools/cli_drivers_ab.py --run head --out profiles/cli_drivers_ab.jsonl
"""
import hashlib
import os
import shutil
import tempfile

import numpy as np

STEPS = 6
LOOP = ["--size", "64", "--step", str(STEPS), "--n_mean_latent", "200", "--batch", "4", "--seed", "0"]


def face_landmarks(shift):
    """A [68,2] set in a 64^2 image whose five ArcFace points are the template at 0.45 x, moved by `shift` pixels."""
    from morphganformer_amd.drivers import ARCFACE_TEMPLATE
    five = ARCFACE_TEMPLATE * 0.45 + 6.0 + shift
    lm = np.random.default_rng(5).uniform(6, 58, (68, 2))
    lm[36:42], lm[42:48], lm[30], lm[48], lm[54] = five[0], five[1], five[2], five[3], five[4]
    return lm


def inputs(root, facenet=False):
    """Everything a command reads, made on the host: the snapshot, two images, two latents, the landmark files, the pair list, a latent tree;
    facenet: also the seed-0 InceptionResnetV1 weights as a plain state dict and as a checkpoint that keeps it under `state_dict`."""
    from PIL import Image
    from morphganformer_amd import drivers, loader
    from morphganformer_amd.synth_weights import TINY, make_state_dict, synthetic_latents
    sd = make_state_dict(TINY, seed=3)
    kw = dict(z_dim=TINY.z_dim, c_dim=0, w_dim=TINY.w_dim, k=TINY.k, img_resolution=TINY.img_resolution, img_channels=3,
              synthesis_kwargs=dict(channel_base=TINY.channel_base, channel_max=TINY.channel_max, end_res=TINY.attn_max_log2res),
              mapping_kwargs=dict(num_layers=TINY.mapping_layers))
    p = lambda *names: os.path.join(root, *names)
    os.makedirs(p("src"))
    loader.save_snapshot_like_reference(p("net.pkl"), {"G": sd, "D": {"b4.fc.weight": np.zeros((2, 3), np.float32)}, "Gs": sd},
                                        {"G": "Generator", "D": "Discriminator", "Gs": "Generator"}, {"G": kw, "Gs": kw})
    yy, xx = np.mgrid[0:64, 0:64]
    for j, name in enumerate(("a.png", "b.png")):                          # smooth colour fields with a blob where the landmarks put the face
        blob = np.exp(-((xx - 30 - 3 * j) ** 2 + (yy - 34) ** 2) / 200.0)
        rgb = np.stack([0.5 + 0.4 * np.sin(xx / (7.0 + j)), 0.2 + 0.7 * blob, 0.5 + 0.4 * np.cos(yy / (5.0 + 2 * j))], axis=2)
        Image.fromarray(np.uint8(np.clip(rgb, 0, 1) * 255)).save(p("src", name))
    lat = synthetic_latents(TINY, 2, seed=11)
    for j, name in enumerate(("a.mat", "b.mat")):
        drivers.save_latent_mat(p(name), lat[j:j + 1])
        drivers.save_latent_mat(p("tree", "id0", "xy"[j], name), lat[j:j + 1])
    la, lb = face_landmarks(0.0), face_landmarks(2.0)
    steps = np.stack([la + 0.25 * i for i in range(STEPS)])
    np.savez(p("lm.npz"), target=la, steps=steps, target_b=lb)
    rng = np.random.Generator(np.random.PCG64(77))
    base = np.unique(np.stack([rng.integers(8, 56, 68), rng.integers(8, 56, 68)], axis=1), axis=0)
    np.savez(p("warp.npz"), lm1=base + rng.integers(-2, 3, base.shape), lm2=base + rng.integers(-2, 3, base.shape), lm_G=base + rng.integers(-3, 4, base.shape))
    with open(p("pairs.csv"), "w") as f:
        f.write("img1,img2,simi\na.png,b.png,0.9\n")
    if facenet:
        import torch
        from morphganformer_amd.facenet import random_state
        state = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in random_state(0).items()}
        torch.save(state, p("facenet.pth"))
        torch.save({"state_dict": state, "epoch": 1}, p("facenet_wrapped.pth"))
    return p


def config(name, argv):
    """argv: the command line with {name} for an input file and {out} for the directory the command writes into."""
    def run(Recorder):
        import torch
        from morphganformer_amd import cli
        root = os.path.join(tempfile.gettempdir(), "cli_drivers_ab")           # one fixed place: extract-facenet stores the paths it was given
        shutil.rmtree(root, ignore_errors=True)
        try:
            p = inputs(root, facenet=any("facenet" in a and a.endswith(".pth}") for a in argv))
            out = p("out")
            os.makedirs(out)
            args = [a.replace("{out}", out) if "{out}" in a else (p(*a[1:-1].split("/")) if a.startswith("{") else a) for a in argv]
            torch.manual_seed(3)                                 # keys the generator's per-layer noise stream (noise_mode="random")
            with Recorder() as rec:
                try:
                    code = cli.main(args)
                except (Exception, SystemExit) as e:             # a command that refuses its arguments is a result too; a GPU fault is not caught
                    code = f"{type(e).__name__}: {e}"[:300]
                torch.cuda.synchronize()
            files = {}
            for d, _, names in sorted(os.walk(out)):
                for n in sorted(names):
                    with open(os.path.join(d, n), "rb") as f:
                        data = f.read()
                    if n.endswith(".mat"):                       # a MAT-file opens with 128 bytes of text that hold its creation time
                        data = data[128:]
                    files[os.path.relpath(os.path.join(d, n), out)] = hashlib.sha256(data).hexdigest()[:16]
            return {"recorder": rec, "exit": code, "n_files": len(files), "files": files}
        finally:
            shutil.rmtree(root, ignore_errors=True)
    return name, run


def configs():
    proj = lambda name, *more: config("project/" + name, ["project", "--model", "{net.pkl}", "--image", "{src/a.png}", "--path_to_gen", "{out}/p", *LOOP, *more])
    morph = lambda name, *more: config(name, ["morph", "--model", "{net.pkl}", "--w1", "{a.mat}", "--w2", "{b.mat}", "--out", "{out}/m/a+b", *more])
    refine = ["--alphas", "0.25,0.5", "--refine", "--image-a", "{src/a.png}", "--image-b", "{src/b.png}", "--size", "64", "--step", str(STEPS),
              "--n_mean_latent", "200", "--seed", "0", "--lpips-random-backbone", "--biometric", "iresnet18", "--biometric-random", "--gamma", "0.1",
              "--id-balance", "0.05", "--id-metric", "cosine", "--truncation_psi", "0.5"]    # (cosine: a random embedder's distance stays under min_loss's 100)
    rand = "--lpips-random-backbone"
    return [
        config("generate", ["generate", "--model", "{net.pkl}", "--output-dir", "{out}/g", "--images-num", "2", "--seed", "1"]),
        proj("literal", "--no-lpips", "--landmarks", "{lm.npz}"),
        proj("gradient", "--mode", "gradient", "--no-lpips", "--landmarks", "{lm.npz}", "--w_plus"),
        proj("lpips_random_backbone", rand),
        proj("biometric_align", "--no-lpips", "--biometric", "iresnet18", "--biometric-random", "--biometric-align", "--landmarks", "{lm.npz}", "--gamma", "1e-3",
             "--min-loss-init", "1e30"),
        proj("mdf_random", "--no-lpips", "--mdf-random", "--mdf-scales", "2"),
        proj("region_from_landmarks", rand, "--landmarks", "{lm.npz}", "--region-from-landmarks", "1,0.1,2"),
        proj("pool_above", rand, "--pool-above", "32"),
        proj("lpips_map", rand, "--lpips-map"),
        proj("optimize_noise", rand, "--mode", "gradient", "--optimize-noise", "--noise_regularize", "1", "--min-loss-init", "1e30"),
        morph("morph", "--alphas", "0,0.5,1", "--truncation_psi", "0.5"),
        morph("morph_refine/lockstep", *refine),
        morph("morph_refine/no_lockstep", *refine, "--no-lockstep"),
        config("morph-pairs", ["morph-pairs", "--model", "{net.pkl}", "--csv", "{pairs.csv}", "--src", "{src}", "--dst-raw", "{out}/raw",
                               "--dst-morph", "{out}/morph", *LOOP, rand]),
        config("morph-tree", ["morph-tree", "--model", "{net.pkl}", "--src", "{tree}", "--dst", "{out}/t"]),
        config("warp", ["warp", "--model", "{net.pkl}", "--w1", "{a.mat}", "--w2", "{b.mat}", "--landmarks", "{warp.npz}", "--out", "{out}/w"]),
        config("lpips-map", ["lpips-map", "--image-a", "{src/a.png}", "--image-b", "{src/b.png}", "--out", "{out}/map", "--size", "64", rand]),
        config("extract-facenet", ["extract-facenet", "{src/a.png}", "{src/b.png}", "--out", "{out}/f.mat", "--biometric-random"]),
        config("extract-facenet/weights", ["extract-facenet", "{src/a.png}", "{src/b.png}", "--out", "{out}/f.mat", "--biometric-weights", "{facenet.pth}"]),
        # the one intended difference: the parent refuses this file (its reader does not unwrap), the refactored tree gives the features of the two rows above
        config("extract-facenet/wrapped", ["extract-facenet", "{src/a.png}", "{src/b.png}", "--out", "{out}/f.mat", "--biometric-weights",
                                           "{facenet_wrapped.pth}"]),
    ]
