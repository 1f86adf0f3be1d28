"""CPU: the float64 restatement of the aligned face crop (tests/face_crop_torch_ref.py) against closed forms, the host-side alignment
(drivers.arcface_crop, drivers.scale_crop), the command line's refusals and the ABI surface of csrc/face_crop.hip.  No kernel is launched."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from face_crop_torch_ref import face_crop_torch, face_crop_torch_adjoint, similarity, subsamples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = similarity(7.3, 4.0, 130.0, 60.0).numpy()            # a typical face in a 1024^2 frame


def _image(n, h, w, seed):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def block_mean_matrix(k):
    return torch.tensor([[k, 0, k / 2 - 0.5], [0, k, k / 2 - 0.5]], dtype=torch.float64)


def test_reference_identity_matrix_returns_the_image():
    x = _image(2, 112, 112, 0)
    eye = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    for filt in ("area", "bilinear"):
        err = float((face_crop_torch(x, eye, 112, filt) - x).abs().max())
        print(filt, "identity error", err)
        assert err <= 1e-12


def test_reference_is_the_block_mean():
    k = 4
    x = _image(1, 112 * k, 112 * k, 1)
    assert subsamples(block_mean_matrix(k)) == k
    err = float((face_crop_torch(x, block_mean_matrix(k), 112) - torch.nn.functional.avg_pool2d(x, k)).abs().max())
    print("block mean error", err)
    assert err <= 1e-12


def test_reference_subsample_counts_and_zero_border():
    assert [subsamples(similarity(s, 10.0, 0, 0)) for s in (0.5, 1.0, 1.3, 2.6, 7.3, 15.9, 40.0)] == [1, 1, 2, 3, 8, 16, 16]
    assert subsamples(similarity(7.3, 0, 0, 0), "bilinear") == 1
    x = torch.ones(1, 3, 20, 20, dtype=torch.float64)
    y = face_crop_torch(x, torch.tensor([[1.0, 0, -30.0], [0, 1.0, 0]], dtype=torch.float64), 16, "bilinear")     # wholly left of the source
    assert float(y.abs().max()) == 0.0
    y = face_crop_torch(x, torch.tensor([[1.0, 0, -0.5], [0, 1.0, 0]], dtype=torch.float64), 16, "bilinear")      # half a pixel over the border
    assert abs(float(y[0, 0, 3, 0]) - 0.5) < 1e-12 and abs(float(y[0, 0, 3, 1]) - 1.0) < 1e-12


def test_reference_adjoint_is_the_adjoint():
    x, m = _image(2, 40, 56, 2), torch.stack([similarity(1.3, 10.0, 4.0, 2.0), similarity(2.6, -5.0, -3.0, 1.0)])
    dy = _image(2, 24, 24, 3)
    lhs = float((face_crop_torch(x, m, 24) * dy).sum())
    rhs = float((x * face_crop_torch_adjoint(dy, m, 40, 56)).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def _five(M):
    from morphganformer_amd.drivers import ARCFACE_TEMPLATE
    return ARCFACE_TEMPLATE @ M[:, :2].T + M[:, 2]


def test_arcface_crop_recovers_a_known_similarity_from_five_points():
    from morphganformer_amd.drivers import arcface_crop
    got = arcface_crop(_five(KNOWN))
    assert got.shape == (2, 3) and got.dtype == np.float64
    print("five points: error", np.abs(got - KNOWN).max())
    assert np.abs(got - KNOWN).max() <= 1e-9
    half = arcface_crop(_five(KNOWN), size=56)                  # the template scales with the crop: twice the source step per crop pixel
    assert np.abs(half[:, :2] - 2 * KNOWN[:, :2]).max() <= 1e-9 and np.abs(half[:, 2] - KNOWN[:, 2]).max() <= 1e-9


def test_arcface_crop_from_68_points():
    """A 68-point set built to have exactly those five points: eye rings whose means are the eye centres, nose tip 30, mouth corners 48 and 54."""
    from morphganformer_amd.drivers import arcface_crop
    five = _five(KNOWN)
    rng = np.random.default_rng(0)
    lm = rng.uniform(100, 900, (68, 2))
    for rows, centre in ((slice(36, 42), five[0]), (slice(42, 48), five[1])):
        ring = rng.standard_normal((6, 2)) * 9.0
        lm[rows] = centre + ring - ring.mean(0)
    lm[30], lm[48], lm[54] = five[2], five[3], five[4]
    got = arcface_crop(lm)
    print("68 points: error", np.abs(got - KNOWN).max())
    assert np.abs(got - KNOWN).max() <= 1e-9
    assert np.abs(arcface_crop(torch.from_numpy(lm)) - got).max() == 0.0
    for bad in (np.zeros((4, 2)), np.zeros((68, 3)), np.full((5, 2), np.nan)):
        with pytest.raises(ValueError, match="arcface_crop"):
            arcface_crop(bad)


def test_arcface_crop_never_returns_a_reflection():
    from morphganformer_amd.drivers import arcface_crop
    rng = np.random.default_rng(1)
    mirrored = _five(KNOWN) * np.array([-1.0, 1.0]) + np.array([1023.0, 0.0])          # the face seen in a mirror: the best fit would flip
    for pts in [mirrored] + [rng.uniform(0, 1024, (5, 2)) for _ in range(50)]:
        lin = arcface_crop(pts)[:, :2]
        assert np.linalg.det(lin) > 0
        assert abs(lin[0, 0] - lin[1, 1]) <= 1e-9 * np.abs(lin).max() and abs(lin[0, 1] + lin[1, 0]) <= 1e-9 * np.abs(lin).max()    # scale * rotation


def test_scale_crop_agrees_with_cropping_the_block_mean():
    """Integer-aligned: M = [[8,0,3.5+16],[0,8,3.5+8]] takes whole 8 x 8 blocks of the image, so the crop of the image equals the crop of its
    4 x 4 block mean under scale_crop(M, 4) = [[2,0,0.5+4],[0,2,0.5+2]], whole 2 x 2 blocks of the pooled image."""
    from morphganformer_amd.drivers import scale_crop
    M = np.array([[8.0, 0.0, 3.5 + 16.0], [0.0, 8.0, 3.5 + 8.0]])
    Ms = scale_crop(M, 4)
    assert np.array_equal(Ms, np.array([[2.0, 0.0, 4.5], [0.0, 2.0, 2.5]])) and np.array_equal(M[:, 2], [19.5, 11.5])     # (a copy, M untouched)
    x = _image(1, 160, 192, 4)
    full = face_crop_torch(x, M, 16)
    pooled = face_crop_torch(torch.nn.functional.avg_pool2d(x, 4), Ms, 16)
    print("scale_crop error", float((full - pooled).abs().max()))
    assert float((full - pooled).abs().max()) <= 1e-12
    both = scale_crop(np.stack([M, KNOWN]), 2)
    assert both.shape == (2, 2, 3) and np.allclose(both[1, :, :2], KNOWN[:, :2] / 2) and np.allclose(both[1, :, 2], (KNOWN[:, 2] + 0.5) / 2 - 0.5)
    assert np.array_equal(scale_crop(M, 1), M)


def test_cli_refusals(tmp_path):
    """--biometric-align is checked before anything is loaded: no model file is read, no GPU is touched."""
    from morphganformer_amd import cli
    lm = tmp_path / "lm.npz"
    np.savez(lm, target=np.zeros((68, 2)), steps=np.zeros((1, 68, 2)))
    base = ["project", "--model", "missing.pkl", "--image", "missing.png", "--biometric-align"]
    with pytest.raises(SystemExit, match="needs --biometric iresnetNN or mobilefacenet"):
        cli.main(base + ["--landmarks", str(lm)])
    with pytest.raises(SystemExit, match="needs --biometric iresnetNN or mobilefacenet"):
        cli.main(base + ["--landmarks", str(lm), "--biometric", "none"])
    with pytest.raises(SystemExit, match="facenet scores the un-cropped frame"):
        cli.main(base + ["--landmarks", str(lm), "--biometric", "facenet", "--biometric-random"])
    with pytest.raises(SystemExit, match="needs --landmarks"):
        cli.main(base + ["--biometric", "iresnet18", "--biometric-random"])
    with pytest.raises(SystemExit, match="does not exist"):
        cli.main(base + ["--biometric", "mobilefacenet", "--biometric-random", "--landmarks", str(tmp_path / "absent.npz")])
    morph = ["morph", "--model", "missing.pkl", "--w1", "a.mat", "--w2", "b.mat", "--out", str(tmp_path / "o"), "--biometric-align"]
    with pytest.raises(SystemExit, match="belongs to --refine"):
        cli.main(morph + ["--biometric", "iresnet18"])
    with pytest.raises(SystemExit, match="needs --biometric iresnetNN or mobilefacenet"):
        cli.main(morph + ["--refine", "--landmarks", str(lm)])
    with pytest.raises(SystemExit, match="facenet scores the un-cropped frame"):
        cli.main(morph + ["--refine", "--landmarks", str(lm), "--biometric", "facenet"])
    with pytest.raises(SystemExit, match="needs --landmarks"):
        cli.main(morph + ["--refine", "--biometric", "iresnet50"])
    with pytest.raises(SystemExit):                              # argparse's own refusal of an unknown filter
        cli.build_parser().parse_args(base + ["--biometric-crop-filter", "lanczos"])
    a = cli.build_parser().parse_args(base + ["--landmarks", str(lm), "--biometric", "iresnet18"])
    assert cli.align_arguments(a) is True and a.biometric_crop_filter == "area"
    a = cli.build_parser().parse_args(base[:-1] + ["--biometric", "facenet"])
    assert cli.align_arguments(a) is False                       # without the flag nothing is checked, nothing changes


def test_symbols_are_declared_exported_and_bound():
    from morphganformer_amd import _lib, build
    build.build()
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "mgf.h")).read()
    declared = set(re.findall(r"\b(mgf_[a-z0-9_]+)\s*\(", hdr))
    for name in ("mgf_face_crop_f32", "mgf_face_crop_bwd_f32", "mgf_face_crop_check"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "face_crop.hip" in build.SOURCES
    assert re.search(r"MGF_CROP_AREA\s*=\s*0,\s*MGF_CROP_BILINEAR\s*=\s*1", hdr)


def test_matrix_check_and_argument_refusals_on_the_host():
    """mgf_face_crop_check reads HOST matrices; the launch entry points refuse bad scalar arguments before any launch."""
    from morphganformer_amd import _lib, build
    build.build()
    lib = _lib.lib()

    def check(m, filt=0):
        m = np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(-1, 2, 3))
        return lib.mgf_face_crop_check(m.ctypes.data, m.shape[0], filt)

    assert check(KNOWN) == 0 and check(np.stack([KNOWN, similarity(0.5, 0, 0, 0).numpy()])) == 0
    assert check(similarity(15.9, 30.0, 0, 0)) == 0                                            # S = 16: the largest the area filter takes
    assert check(similarity(16.1, 0, 0, 0)) == -1 and b"16" in lib.mgf_last_error()            # S would be 17
    assert check(similarity(16.1, 0, 0, 0), 1) == 0                                            # ... which the bilinear filter never forms
    assert check([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]]) == -1 and b"singular" in lib.mgf_last_error()
    assert check([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]], 1) == -1
    assert check(np.stack([KNOWN, np.zeros((2, 3))])) == -1 and b"matrix 1" in lib.mgf_last_error()
    assert check([[1.0, 0.0, math.nan], [0.0, 1.0, 0.0]]) == -1 and b"non-finite" in lib.mgf_last_error()
    assert check(KNOWN, 7) == -1 and lib.mgf_face_crop_check(None, 1, 0) == -1
    # the launch entry points (fake non-null pointers: refused before anything is dereferenced or launched)
    p = ctypes.c_void_p(64)
    assert lib.mgf_face_crop_f32(None, p, p, 1, 8, 8, 112, 1, 0, None) == -1
    assert lib.mgf_face_crop_f32(p, p, p, 2, 8, 8, 112, 3, 0, None) == -1 and b"matrices" in lib.mgf_last_error()
    assert lib.mgf_face_crop_f32(p, p, p, 1, 8, 8, 112, 1, 2, None) == -1 and b"filter" in lib.mgf_last_error()
    assert lib.mgf_face_crop_bwd_f32(p, p, p, 1, 0, 8, 112, 1, 0, 0, None) == -1
    assert lib.mgf_face_crop_bwd_f32(p, p, None, 1, 8, 8, 112, 1, 0, 1, None) == -1


def test_python_layers_name_the_arguments():
    import inspect
    from morphganformer_amd import drivers
    from morphganformer_amd.biometric import BiometricLoss
    from morphganformer_amd.embedder import ArcFaceEmbedder, FaceEmbedder
    from morphganformer_amd.iresnet import IResNetEmbedder
    from morphganformer_amd.mobilefacenet import MobileFaceNetEmbedder
    from morphganformer_amd.projection import GradientProjectionEngine, ProjectionEngine
    assert list(inspect.signature(ArcFaceEmbedder.set_crop).parameters) == ["self", "matrices", "filter"]
    assert list(inspect.signature(BiometricLoss.set_crop).parameters) == ["self", "pred", "target", "target_b", "filter"]
    assert inspect.signature(BiometricLoss.set_crop).parameters["filter"].default == "area"
    assert not hasattr(FaceEmbedder, "set_crop") and callable(BiometricLoss.forget_target) and callable(ArcFaceEmbedder.check_crop)
    for cls in (IResNetEmbedder, MobileFaceNetEmbedder):
        assert "_crop" in cls._MUTABLE                         # clone_for leaves it out: a clone starts without a crop
    assert "face_crop" in inspect.signature(drivers.project_image).parameters
    assert {"face_crop", "face_crop_b"} <= set(inspect.signature(drivers.refine_morph).parameters)
    assert "face_crops" in inspect.signature(drivers.project_many).parameters
    for eng in (ProjectionEngine, GradientProjectionEngine):
        assert "face_crop" in inspect.signature(eng.__init__).parameters
    assert "face_crop" in inspect.signature(ProjectionEngine.retarget).parameters
    with pytest.raises(ValueError, match="landmarks"):
        drivers._resolve_crop("landmarks", None, "face_crop")
    with pytest.raises(ValueError, match="face_crop"):
        drivers._resolve_crop("eyes", np.zeros((68, 2)), "face_crop")
