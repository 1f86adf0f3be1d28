"""The biometric term of the projection objective: the embedding distance the drivers build from a face
embedder (`embedder.FaceEmbedder`: facenet.py, iresnet.py, mobilefacenet.py)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, misc


class BiometricLoss:
    """loss[i] = MSE(embed(pred[i]), embed(target)) like `MSE(img_gen_fea, img_fea)` (1024_example_FaceNet_percept.py:147-158);
    the target embedding is computed once per target (the reference recomputes it every step)."""

    PAIR_METRICS = {"mse": 0, "cosine": 1}

    def __init__(self, embedder="iresnet50", **kw):
        """embedder: an embedder object (IResNetEmbedder, facenet.InceptionResnetV1Embedder) or a name -- "facenet": the network the
        driver scores with, on the un-resized image (1024_example_FaceNet_percept.py:30-32,147-158); "iresnet18/34/50/100": the vendored
        ArcFace network on a 112x112 resize (backbones/iresnet.py); "mobilefacenet": the vendored MobileFaceNet, same contract at ~0.45 GFLOP
        per image (backbones/mobilefacenet.py).  kw (state=, n=, device=, seed=) go to the embedder's constructor."""
        if isinstance(embedder, str):
            if embedder == "facenet":
                from .facenet import InceptionResnetV1Embedder
                embedder = InceptionResnetV1Embedder(**kw)
            elif embedder == "mobilefacenet":
                from .mobilefacenet import MobileFaceNetEmbedder
                embedder = MobileFaceNetEmbedder(**kw)
            elif embedder.startswith("iresnet"):
                from .iresnet import IResNetEmbedder
                embedder = IResNetEmbedder(depth=int(embedder[len("iresnet"):]), **kw)
            else:
                raise ValueError(f"unknown embedder {embedder!r} (facenet, iresnet18/34/50/100, mobilefacenet)")
        self.embedder = embedder
        self._target = None                       # [nt, EMB] of set_target
        self._target_stride = 0
        self._tgt_net, self._tgt_nt = None, None
        self._scratch = None
        self._pair, self._pair_bufs, self._pair_scale, self._pair_dummy = None, None, None, None
        self._demb = None                         # [n, EMB]: the embedding gradient handed to the embedder's backward
        self.pair_trace = None
        self._crop = None                         # set_crop's dict(target=, target_b=, filter=); the candidates' matrices live in the embedder
        self._target_src = None                   # the arguments of the latest set_target / set_target_pair: set_crop re-embeds from them

    def set_crop(self, pred, target=None, target_b=None, filter="area"):
        """Embed through the aligned face crop of `ArcFaceEmbedder.set_crop` instead of the plain resize.  pred: the matrix [2,3] (or B matrices
        [B,2,3], lockstep) of the candidates; target / target_b: the matrices under which set_target / set_target_pair embed the target
        image(s), each pred by default.  None for pred restores the resize everywhere.  Call it before set_target*.  The FaceNet embedder scores
        the un-cropped frame by the reference's definition: MgfError.

        Stored target embeddings never belong to another crop than the one in force.  When a target is already set, it is embedded again here
        FROM THE TENSORS set_target* WAS HANDED -- this object keeps references to them, not copies, and reads what they hold now -- provided
        the new target matrices can apply to it (one matrix, or as many as it has images); a remembered target they cannot apply to (another
        batch size: a BiometricLoss handed from one engine to the next) is dropped with its embeddings, and set_target* must be called again.
        A caller that is about to call set_target* anyway says so with forget_target() first and saves the embedder pass.  Every matrix is
        checked before anything is changed: a refused matrix leaves the crop, the embedder and the stored embeddings as they were."""
        from .embedder import ArcFaceEmbedder
        if not isinstance(self.embedder, ArcFaceEmbedder):
            raise _lib.MgfError(f"set_crop: {type(self.embedder).__name__} takes no face crop (the ArcFace embedders iresnet*/mobilefacenet do)")
        crop, counts = None, ()
        if pred is not None:
            crop = dict(target=pred if target is None else target, target_b=pred if target_b is None else target_b, filter=filter)
            ArcFaceEmbedder.check_crop(pred, filter)
            counts = [ArcFaceEmbedder.check_crop(crop[k], filter)[0].shape[0] for k in ("target", "target_b")]
        self.embedder.set_crop(pred, filter)
        self._crop = crop
        if self._target_src is None:
            return
        setter, args = self._target_src
        nt = int(args[0].shape[0])
        if any(c not in (1, nt) for c in (counts if self._pair is not None else counts[:1])):
            self.forget_target()
            self._target, self._pair, self.pair_trace = None, None, None
            return
        trace = self.pair_trace
        setter(*args)
        self.pair_trace = trace

    def forget_target(self):
        """Drop the references to the target tensors of the latest set_target* call (set_crop re-embeds from them).  The stored embeddings stay:
        for a caller that calls set_target* next, such as an engine that was just handed this object or is being re-targeted."""
        self._target_src = None

    def _embed_target(self, net, image, which):
        if self._crop is not None:               # the target net is a clone: it starts without a crop and is only ever given one here
            net.set_crop(self._crop[which], self._crop["filter"])
        elif getattr(net, "_crop", None) is not None:
            net.set_crop(None)
        return net.embed_image(image.float())

    def _target_net(self, nt):
        """The embedder of the target images: an instance sharing nothing mutable with the candidates' workspace."""
        if self._tgt_net is None or self._tgt_nt != nt:
            self._tgt_net, self._tgt_nt = self.embedder.clone_for(nt), nt
        return self._tgt_net

    def _demb_for(self, n, device):
        if self._demb is None or self._demb.shape[0] != n:
            self._demb = torch.empty(n, self.embedder.EMB, dtype=torch.float32, device=device)
        return self._demb

    def set_target(self, target):
        """One target [1,3,H,W] shared by every candidate, or B targets that pair up with B candidates (lockstep projections)."""
        nt = int(target.shape[0])
        emb = self._embed_target(self._target_net(nt), target, "target")
        self._target_src = (self.set_target, (target,))
        if self._target is not None and self._target.shape == emb.shape:
            self._target.copy_(emb)   # in place: a captured hipGraph of the projection engine keeps reading this buffer (ProjectionEngine.retarget)
        else:
            self._target = emb.clone()
        self._target_stride = self.embedder.EMB if nt > 1 else 0
        self._pair, self.pair_trace = None, None

    def set_target_pair(self, target_a, target_b, alpha, id_balance=0.0, metric="mse"):
        """Two identities per candidate (morph refinement): distance_into / grad_into then score
            scale * ((1 - alpha) d_a + alpha d_b) + id_balance * |d_a - d_b|,   d_t = d(embed(pred), embed(target_t))
        in ONE launch of mgf_embed_pair_loss_f32 -- metric "mse": d = mean (e - t)^2, today's term; "cosine": 1 - cosine_similarity(e, t), the
        distance ArcFace embedders are trained for.  target_b carries alpha, target_a 1 - alpha (merge_morph's convention).  targets [1,3,H,W],
        or [B,...] for B lockstep pairs; alpha a float or B of them.  Both embeddings are computed once, here; with unchanged geometry the
        buffers are rewritten in place (a captured hipGraph keeps reading them).  `pair_trace` = (float64 tensor [n, rows, 2], int32 device
        step counter) makes every distance_into call record (d_a, d_b) in the counter's row.  A later set_target() clears the pair."""
        if metric not in self.PAIR_METRICS:
            raise ValueError(f"set_target_pair: metric must be 'mse' or 'cosine' (got {metric!r})")
        if tuple(target_a.shape) != tuple(target_b.shape):
            raise ValueError(f"set_target_pair: the two targets differ in shape: {tuple(target_a.shape)} vs {tuple(target_b.shape)}")
        nt = int(target_a.shape[0])
        al = misc.as_numpy(alpha, np.float64).reshape(-1)
        if al.size not in (1, nt) or not np.all((al >= 0.0) & (al <= 1.0)):
            raise ValueError(f"set_target_pair: alpha must be one value or {nt} values in [0, 1] (got {alpha!r})")
        al = np.array(np.broadcast_to(al, (nt,)))
        net = self._target_net(nt)
        ea = self._embed_target(net, target_a, "target").clone()
        eb = self._embed_target(net, target_b, "target_b")
        self._target_src = (self.set_target_pair, (target_a, target_b, alpha, id_balance, metric))
        old = self._pair_bufs
        if old is None or old[0].shape != ea.shape:
            old = self._pair_bufs = (torch.empty_like(ea), torch.empty_like(ea), torch.empty(nt, dtype=torch.float32, device=ea.device))
        old[0].copy_(ea)
        old[1].copy_(eb)
        old[2].copy_(torch.as_tensor(al, dtype=torch.float32))
        self._pair = dict(ta=old[0], tb=old[1], alpha=old[2], delta=float(id_balance), metric=self.PAIR_METRICS[metric], alpha_n={})
        self._target_stride = self.embedder.EMB if nt > 1 else 0
        self._pair_scale, self.pair_trace = None, None

    def _pair_launch(self, out, emb, n, scale, accumulate, with_trace):
        P = self._pair
        alpha = P["alpha"]
        if alpha.numel() != n:                      # one shared pair, n candidates: every candidate reads the same weight
            alpha = P["alpha_n"].get(n)
            if alpha is None:
                alpha = P["alpha_n"][n] = P["alpha"].expand(n).contiguous()
        demb = self._demb_for(n, emb.device)
        trace = step = None
        rows = 0
        if with_trace and self.pair_trace is not None:
            trace, step = self.pair_trace
            assert trace.dtype == torch.float64 and trace.shape[0] == n and trace.shape[2] == 2 and trace.is_contiguous()
            rows = int(trace.shape[1])
        _lib.check(_lib.lib().mgf_embed_pair_loss_f32(out.data_ptr(), demb.data_ptr(), _lib.ptr(trace), emb.data_ptr(), P["ta"].data_ptr(),
                                                      P["tb"].data_ptr(), alpha.data_ptr(), n, self.embedder.EMB, self._target_stride, float(scale),
                                                      P["delta"], P["metric"], int(accumulate), _lib.ptr(step), rows, _lib.stream_ptr()),
                   "embed_pair_loss")
        self._pair_scale = float(scale)

    def distance_into(self, out, pred, scale=1.0, accumulate=False):
        """out[i] (+)= scale * mean((embed(pred[i]) - embed(target))^2);  out: float32 [n].  With a target pair (set_target_pair): the pair
        objective, its embedding gradient kept for grad_into."""
        n = pred.shape[0]
        if self._pair is not None:
            assert self._target_stride == 0 or self._pair["ta"].shape[0] == n, "B target pairs pair up with B candidates"
            self._pair_launch(out, self.embedder.embed_image(pred), n, scale, accumulate, True)
            return out
        assert self._target is not None, "call set_target first (set_crop drops a target its matrices cannot apply to)"
        assert self._target_stride == 0 or self._target.shape[0] == n, "B targets pair up with B candidates"
        emb = self.embedder.embed_image(pred)
        need = n * int(_lib.lib().mgf_reduce_scratch_floats())
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float32, device=emb.device)
        _lib.check(_lib.lib().mgf_mse_f32(out.data_ptr(), emb.data_ptr(), self._target.data_ptr(), n, self.embedder.EMB, self._target_stride,
                                          float(scale), int(accumulate), self._scratch.data_ptr(), _lib.stream_ptr()), "mse(embedding)")
        return out

    def grad_into(self, dimg, scale=1.0, accumulate=False):
        """dimg (+)= d(scale * distance)/d(pred) for the pred of the latest distance_into call (gradient mode)."""
        e = self.embedder
        n = e.n
        if self._pair is not None:
            if self._pair_scale != float(scale):    # another coefficient than distance_into's: the same launch again, its value discarded
                if self._pair_dummy is None or self._pair_dummy.numel() != n:
                    self._pair_dummy = torch.zeros(n, dtype=torch.float32, device=dimg.device)
                self._pair_launch(self._pair_dummy, e.out, n, scale, False, False)
            return e.backward(self._demb, dimg, accumulate)
        demb = self._demb_for(n, dimg.device)
        _lib.check(_lib.lib().mgf_mse_grad_f32(demb.data_ptr(), e.out.data_ptr(), self._target.data_ptr(), n, e.EMB, self._target_stride,
                                               float(scale), 0, _lib.stream_ptr()), "mse_grad(embedding)")
        return e.backward(demb, dimg, accumulate)

    def __call__(self, pred, target):
        self.set_target(target)
        out = torch.zeros(pred.shape[0], dtype=torch.float32, device=pred.device)
        return self.distance_into(out, pred)
