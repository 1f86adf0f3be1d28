"""Host side of the face embedders' shared base (embedder.py, biometric.py): the seeded stand-in weights every GPU test and the bench run on
are pinned by hash (one reordered draw would silently move every number), BatchNorm folding is the formula in float64, the classes implement
the written contract.  No device."""
import hashlib

import numpy as np
import pytest
import torch


def _state_hash(sd):
    m = hashlib.sha256()
    for k in sorted(sd):
        v = np.ascontiguousarray(sd[k])
        for part in (k.encode(), str(v.dtype).encode(), str(v.shape).encode(), v.tobytes()):
            m.update(part)
    return m.hexdigest()[:16]


# sha256 (first 16 hex digits) of the state dicts as the three modules drew them before they shared `seeded_bn` (numpy 2.2.6, PCG64)
SEEDED = [("iresnet", (18, 0), "4f32166940314360", 156), ("iresnet", (50, 0), "40876c727a1734c9", 396), ("iresnet", (18, 3), "f20dc82008e45026", 156),
          ("mobilefacenet", (0,), "03936bf754d78c9f", 283), ("mobilefacenet", (2,), "7856ad17c6f6e06b", 283),
          ("facenet", (0,), "f08b5c107690de15", 602), ("facenet", (2,), "2c3a27f842c01e63", 602)]


@pytest.mark.parametrize("module,args,digest,keys", SEEDED, ids=lambda v: str(v))
def test_seeded_weights_are_unchanged(module, args, digest, keys):
    import importlib
    sd = importlib.import_module("morphganformer_amd." + module).random_state(*args)
    assert len(sd) == keys
    assert all(v.dtype == np.float32 for v in sd.values())
    assert _state_hash(sd) == digest


def test_biometric_loss_is_one_class_under_both_names():
    from morphganformer_amd import biometric
    from morphganformer_amd.iresnet import BiometricLoss
    assert BiometricLoss is biometric.BiometricLoss


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_bn_affine_is_the_formula_in_float64(eps):
    from morphganformer_amd.embedder import bn_affine
    rng = np.random.Generator(np.random.PCG64(7))
    sd = {"a.bn.weight": rng.uniform(0.5, 1.5, 37).astype(np.float32), "a.bn.bias": rng.standard_normal(37).astype(np.float32),
          "a.bn.running_mean": rng.standard_normal(37).astype(np.float32), "a.bn.running_var": rng.uniform(0.01, 2.0, 37).astype(np.float32),
          "a.bn.num_batches_tracked": np.int64(3)}
    w, b, m, v = (sd["a.bn." + k].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    scale = w / np.sqrt(v + eps)
    shift = b - m * scale
    for state in (sd, {k: torch.from_numpy(np.asarray(x)) for k, x in sd.items()}):
        s, t = bn_affine(state, "a.bn", eps)
        assert s.dtype == np.float64 and t.dtype == np.float64
        assert np.array_equal(s, scale) and np.array_equal(t, shift)


def test_the_three_embedders_implement_the_contract():
    from morphganformer_amd.embedder import ArcFaceEmbedder, FaceEmbedder
    from morphganformer_amd.facenet import InceptionResnetV1Embedder
    from morphganformer_amd.iresnet import IResNetEmbedder
    from morphganformer_amd.mobilefacenet import MobileFaceNetEmbedder
    assert issubclass(IResNetEmbedder, ArcFaceEmbedder) and issubclass(MobileFaceNetEmbedder, ArcFaceEmbedder)
    assert issubclass(InceptionResnetV1Embedder, FaceEmbedder) and not issubclass(InceptionResnetV1Embedder, ArcFaceEmbedder)
    for cls in (IResNetEmbedder, MobileFaceNetEmbedder, InceptionResnetV1Embedder):
        assert cls.EMB == 512 and cls.keep_activations is False
        assert cls.clone_for is FaceEmbedder.clone_for and "out" in cls._MUTABLE
        for name in ("embed_image", "backward", "_alloc", "__call__"):
            assert callable(getattr(cls, name)), (cls, name)
