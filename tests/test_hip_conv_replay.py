"""Every convolution launch the production workloads make, replayed on its own against float64, per element (tests/conv_replay.py).

The full-size suite compares end to end -- losses, images, best steps -- so an error confined to one strip seam, one border column of one
layer or the last K slice of a split-K launch is averaged away before anything looks at it; the per-kernel float64 tests run small shapes
that land on a few leaves of the dispatch tree only.  Here the real workloads are RECORDED (shapes and options of every call of the seven
wrappers of conv.py), and each distinct call is REPLAYED through the same wrapper with the same arguments on seeded random data, so the
dispatcher makes the same choice -- asserted: the (kernel instantiation, ksplit) list of the replay equals the recorded one, record by
record and as a multiset -- and gated at the borders, at both sides of every tile seam and strip end, and on a random fill."""
import collections
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_replay as cr  # noqa: E402

pytestmark = pytest.mark.gpu

# Records that are NOT replayed: (workload, predicate on the record, the existing test that covers it).  At most 5 % of a workload's distinct records.
EXCLUDED = []
FILL = 1024                              # seeded random interior positions per launch: the one part the time budget may shrink


def _replay_all(cv, records, label):
    failures, replayed = [], collections.Counter()
    for sig, recorded in records.items():
        try:
            res = cr.replay(cv, sig, fill=FILL)                   # (data seed: a hash of the record's own signature)
        except cr.Unexpressible as exc:
            failures.append(f"{label}: a record the evaluator cannot express ({exc}): {cr.format_sig(sig)}")
            continue
        replayed[res["launches"]] += 1
        print(f"{label}: {cr.format_sig(sig)} -> {res['launches']} worst {res['worst']:.3f} of c*A, rel {res['rel']:.2e}, r {res['r']:.2e}, "
              f"head-room {res['headroom']:.2f} r ({res['elements']} elements)")
        if res["launches"] != recorded:
            failures.append(f"{label}: the replay launched {res['launches']}, the workload {recorded}: {cr.format_sig(sig)}")
        if not res["ok"]:
            failures.append(f"{label}: {cr.format_sig(sig)}\n   launches (kernel, ksplit) {res['launches']}; worst |got - ref64| = {res['worst']:.3f} c A (c = {res['c']:.3e}, "
                            f"m = {res['m']}), max-norm relative error {res['rel']:.3e} (bound {res['rel_bound']}); worst element {res['where']}; {res['problems']}")
        torch.cuda.empty_cache()
    return failures, replayed


@pytest.mark.parametrize("workload", list(cr.WORKLOADS))
def test_replay_every_launch_of(workload):
    from morphganformer_amd import conv as cv
    t0 = time.time()
    rec = cr.record_workload(cv, workload)
    torch.cuda.empty_cache()
    t1 = time.time()
    assert rec.records, "the workload made no convolution call"
    assert not rec.conflicts, f"one call signature, two different launches: {rec.conflicts[:3]}"
    records = dict(rec.records)
    excluded = [s for s in records if any(w == workload and pred(dict(s)) for w, pred, _ in EXCLUDED)]
    assert len(excluded) <= 0.05 * len(records), (len(excluded), len(records))
    for s in excluded:
        del records[s]
    failures, replayed = _replay_all(cv, records, workload)
    print(f"{workload}: {rec.calls} calls, {len(rec.records)} distinct, recorded in {t1 - t0:.1f} s, replayed in {time.time() - t1:.1f} s")
    assert not failures, "\n".join(failures)
    assert replayed == collections.Counter(records.values()), "the multiset of (kernel, ksplit) launches differs between workload and replay"


def test_persistent_strip_walk_of_4_8_16_32_tiles():
    """No workload on one box pins every strip length: persistent form-3 launches at cin = 32, 1024 x 1024 with 1 / 2 / 4 / 8 images walk
    vertical strips of 4 / 8 / 16 / 32 tiles by the launch code's own rule -- plain, full-resolution residual, half-resolution residual and
    fused ToRGB, through the same replay path (both sides of every strip end at every seam column, see conv_replay.select_positions)."""
    from morphganformer_amd import conv as cv
    failures = []
    for n, case, sig in cr.strip_walk_records():
        strip = cr.wino3_strip(n, 32, 32, 1024, 1024)      # (the launch rule re-stated in Python: a label, the profile does not report the strip)
        assert strip == ("vertical", {1: 4, 2: 8, 4: 16, 8: 32}[n])
        res = cr.replay(cv, sig, fill=FILL)
        print(f"strip walk n={n} {case}: {res['launches']} strip {strip} worst {res['worst']:.3f} of c*A, rel {res['rel']:.2e}, head-room {res['headroom']:.2f} r")
        want = "wino3p_conv_kernel<8, true>" if case == "ToRGB" else "wino3p_conv_kernel<8, false>"
        if res["launches"] != ((want, 1),):
            failures.append(f"n={n} {case}: launched {res['launches']}, not the persistent kernel")
        if not res["ok"]:
            failures.append(f"n={n} {case}: worst {res['worst']:.3f} c A (c = {res['c']:.3e}), rel {res['rel']:.3e}; worst element {res['where']}; {res['problems']}")
        torch.cuda.empty_cache()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tile", list(cr.DIRECT_TILE_CASES))
def test_workgroup_tiles_at_their_smallest_shape(tile):
    """conv_taps_kernel's 1 x 3 and 1 x 4 workgroup tiles (the workloads reach them in gradient mode and the loss networks only) and the
    stride-1 mode of the 1 x 2 and 1 x 1 tiles (which the workloads reach as transposed convs only), each at the smallest shape that selects it
    (DESIGN.md section 4 lists which workloads reach which tile)."""
    from morphganformer_amd import conv as cv
    res = cr.replay(cv, cr.direct_tile_records()[tile], fill=FILL)
    print(f"{tile}: {res['launches']} worst {res['worst']:.3f} of c*A, rel {res['rel']:.2e}, head-room {res['headroom']:.2f} r")
    assert len(res["launches"]) == 1 and res["launches"][0][0].startswith(tile), res["launches"]
    assert res["ok"], (res["worst"], res["rel"], res["where"], res["problems"])


@pytest.mark.parametrize("kind,n,c", cr.MDF_CASES)
def test_mdf_body_launches_at_1024(kind, n, c):
    """The MDF objective's form-3 launches at production shape: the discriminators' body layer (N = 32 / 64 / 128 channels, 1024^2) at 32 candidates
    and at one, and the masked adjoint of gradient mode at one -- called like morphganformer_amd/mdf.py calls them, gated like every replayed
    record (borders of the valid frame, every tile seam and strip end, random fill; the adjoint exactly 0 outside its ring)."""
    from morphganformer_amd import conv as cv
    res = cr.replay_mdf(cv, kind, n, c, fill=FILL)
    print(f"{kind} n={n} N={c}: {res['launches']} strip {res['strip']} worst {res['worst']:.3f} of c*A, rel {res['rel']:.2e}, head-room {res['headroom']:.2f} r")
    assert len(res["launches"]) == 1
    name = res["launches"][0][0]
    want = ("wino3p_conv_kernel<8, false, true>" if c == 32 else "wino3_conv_kernel<1, 1, false, true>") if kind == "mdf_body_backward" else \
        ("wino3p_conv_kernel<8, false>" if c == 32 else None)
    assert want is None or name == want, name
    assert "wino3" in name
    assert res["ok"], (res["worst"], res["rel"], res["rel_bound"], res["where"], res["problems"])
    torch.cuda.empty_cache()
