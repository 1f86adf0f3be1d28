"""Census of the convolution launches: records the production workloads of tests/conv_replay.py (literal loop, generator, gradient mode,
the LPIPS backbones, FaceNet, IResNet-50), replays every distinct call against float64 and prints one line per launch -- workload, wrapper,
shapes, options, kernel instantiation(s) with ksplit, the persistent form's strip, and the worst |got - ref64| / (c A) of its replay.

    python tools/conv_census.py > profiles/conv_launch_census.txt

The committed output is what a reviewer diffs when a dispatch threshold moves."""
import collections
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import conv_replay as cr  # noqa: E402


def main():
    from morphganformer_amd import conv as cv
    assert torch.cuda.is_available(), "the census runs the launches: it needs the GPU"
    head = collections.defaultdict(float)
    kernels = collections.Counter()
    print("# The strip column is COMPUTED from a Python re-statement of csrc/wino3.hip's launch rule (conv_replay.wino3_strip), not observed: the conv profile")
    print("# reports the kernel name and ksplit only.  The transposed conv's border kernel and the narrow kernels (conv3x3_few_outputs, conv3x3s2_few_inputs,")
    print("# the few-outputs transposed conv) are outside the conv profile: a tconv row lists its main launch only, a narrow row lists [] (their VALUES are gated).")
    print("# workload | wrapper call | launches (kernel, ksplit) | strip | worst |got-ref64|/(cA) | head-room |got-ref64|/(rA) | max-norm rel | elements")

    def line(label, sig, res):
        strip = f"{res['strip'][0]} x{res['strip'][1]}" if res["strip"] and any("wino3p" in k for k, _ in res["launches"]) else "-"
        print(f"{label} | {cr.format_sig(sig)} | {list(res['launches'])} | {strip} | {res['worst']:.3f} | {res['headroom']:.2f} | {res['rel']:.2e} | "
              f"{res['elements']}{'' if res['ok'] else ' | FAILED ' + res['where'] + ' ' + str(res['problems'])}")
        head[res["family"]] = max(head[res["family"]], res["headroom"] if res["headroom"] == res["headroom"] else 0.0)
        for k in res["launches"]:
            kernels[k] += 1

    for name in cr.WORKLOADS:
        rec = cr.record_workload(cv, name)
        torch.cuda.empty_cache()
        for sig, recorded in rec.records.items():
            res = cr.replay(cv, sig, fill=1024)                     # (data seed: a hash of the record's signature, as in tests/test_hip_conv_replay.py)
            line(name, sig, res)
            if res["launches"] != recorded:
                print(f"{name} | REPLAY MISMATCH: recorded {list(recorded)}")
            torch.cuda.empty_cache()
    for n, case, sig in cr.strip_walk_records():
        line(f"strip walk n={n} {case}", sig, cr.replay(cv, sig, fill=1024))
    for tile, sig in cr.direct_tile_records().items():
        line(f"direct tile case {tile}", sig, cr.replay(cv, sig, fill=1024))
    for kind, n, c in cr.MDF_CASES:
        line(f"MDF direct case {kind}", (("x", (n, c, 1024, 1024)),), cr.replay_mdf(cv, kind, n, c, fill=1024))
        torch.cuda.empty_cache()
    print("# head-room per kernel family, max |got - ref64| / (r A):")
    for fam, v in sorted(head.items()):
        print(f"#   {fam}: {v:.2f}")
    print("# distinct (kernel, ksplit) and the number of distinct launches on each:")
    for k, c in sorted(kernels.items()):
        print(f"#   {k[0]} ksplit {k[1]}: {c}")


if __name__ == "__main__":
    main()
