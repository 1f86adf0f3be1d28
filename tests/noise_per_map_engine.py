"""The per-map noise path of gradient mode as an independent reference (a helper of tests/test_hip_noise_sets.py, not a test module).

GradientProjectionEngine(optimize_noise=True) runs regulariser, Adam and normalisation as one set call each (mgf_noise_sets_*,
mgf_adam_sets_f32).  `PerMapNoiseEngine` is the same engine, one target, with those two steps restated as loops over the per-map entries
-- other kernels, other scratch, the same [1, total] buffers through the per-layer views -- so that "one target is a set of one" stays a
comparison of two implementations, bit for bit."""
import torch

from morphganformer_amd import _lib
from morphganformer_amd.projection import GradientProjectionEngine


class PerMapNoiseEngine(GradientProjectionEngine):
    def _init_noise(self, noise_init, seed):
        super()._init_noise(noise_init, seed)
        assert self.targets == 1, "the per-map reference is one target's"
        L, dev = _lib.lib(), self.device
        nbytes = max(int(L.mgf_noise_regularize_scratch_bytes(r)) for _, r in self.noise_layers)
        self.per_map_reg_scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        self.per_map_norm_scratch = torch.empty(int(L.mgf_noise_normalize_scratch_bytes()) // 8, dtype=torch.float64, device=dev)

    def _noise_regularize(self, has_p):
        """p_loss (+)= noise_regularize * sum_maps reg and noise_grad += noise_regularize * d reg / d maps, map after map on one stream."""
        L, st, a = _lib.lib(), _lib.stream_ptr(), self.args
        for i, (name, r) in enumerate(self.noise_layers):
            _lib.check(L.mgf_noise_regularize_grad_f32(self.dnoises[name].data_ptr(), self.p_loss.data_ptr(), self.noises[name].data_ptr(), r,
                                                       float(a.noise_regularize), 1, int(has_p or i > 0), self.per_map_reg_scratch.data_ptr(), st),
                       "noise_regularize_grad")

    def _noise_update(self):
        """Keep the maps of an improving step, one elementwise Adam launch over the row, then noise_normalize_ per map."""
        L, st = _lib.lib(), _lib.stream_ptr()
        _lib.check(L.mgf_keep_improvements(self.best_noise_flat.data_ptr(), self.noise_flat.data_ptr(), self.noise_flat.numel(),
                                           self.noise_slot.take.data_ptr(), 1, st), "keep_improvements(noise maps)")
        _lib.check(L.mgf_adam_elementwise_f32(self.noise_flat.data_ptr(), self.noise_m.data_ptr(), self.noise_v.data_ptr(),
                                              self.noise_adam_t.data_ptr(), self.noise_grad.data_ptr(), self.lr_table.data_ptr(),
                                              self.noise_ctr.data_ptr(), _lib.ptr(self.valid), self.noise_flat.numel(), self.steps,
                                              float(self.betas[0]), float(self.betas[1]), self.adam_eps, self.weight_decay, st), "adam_elementwise")
        for name, r in self.noise_layers:
            _lib.check(L.mgf_noise_normalize_f32(self.noises[name].data_ptr(), r * r, self.noise_ctr.data_ptr(), _lib.ptr(self.valid), self.steps,
                                                 self.per_map_norm_scratch.data_ptr(), st), "noise_normalize")
