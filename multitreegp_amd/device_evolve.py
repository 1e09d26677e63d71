"""Device-side evolution step (include/mtgp.h ABI v22, csrc/mtgp_evolve.hip): the population stays
on the GPU between generations.  DeviceEvolver mirrors host.HostEvolver -- the same strategy
parameters packed into the same MtgpEvolveConfig -- and runs the code the host library runs
(csrc/mtgp_evolve_core.h), draw for draw: columns f, a, b bit for bit, values to within 1 float32
ulp where the device's f64 log rounds differently inside a normal draw.

evolve / sample_population enqueue on the current stream and return fresh CUDA tensors from
torch's stream-ordered allocator: an output never aliases an input or memory the caller can still
see.  evolve_host / sample_population_host run the same core code on the CPU, serially, inside
libmtgp_hip.so (the host twins: tests/test_device_evolve_host.py holds them and HostEvolver to the
same recorded digests)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat
from .host import HostEvolver

_U64 = 2**64 - 1


class DeviceEvolver(HostEvolver):
    def __init__(self, library, max_nodes: int, max_init_depth: int, coefficient_sd: float = 1.0,
                 migration_period: int = 10, migration_size: int = 0, tournament_size: int = 7, elite_size: int = 0,
                 tournament_probabilities=None, reproduction_type_probabilities=None,
                 reproduction_probabilities=None, num_populations: int = 1, device=None):
        super().__init__(library, max_nodes, max_init_depth, coefficient_sd, migration_period, migration_size,
                         tournament_size, elite_size, tournament_probabilities, reproduction_type_probabilities,
                         reproduction_probabilities, num_populations)
        self.hip = nat.load()
        self._device_arg = device  # resolved on first use: the constructor and the host twins need no GPU
        self._device = None
        n = self.hip.mtgp_evolve_config_pack(ctypes.addressof(self.cfg), self.num_populations, self.num_trees,
                                             None, 0)
        if n < 0:
            raise ValueError("mtgp_evolve_config_pack rejected the strategy (N <= 256, tournament_size <= 64, "
                             "operand counts 0..2, reproduction probabilities > 0)")
        self._blob_host = np.zeros(n, np.uint8)
        self.hip.mtgp_evolve_config_pack(ctypes.addressof(self.cfg), self.num_populations, self.num_trees,
                                         self._blob_host.ctypes.data, n)
        self._blob = None  # uploaded once, on first use (the constructor needs no GPU)

    @classmethod
    def for_strategy(cls, gp) -> "DeviceEvolver":
        return cls(gp.library, gp.max_nodes, gp.max_init_depth, gp.coefficient_sd, gp.migration_period,
                   gp.migration_size, gp.tournament_size, gp.elite_size, gp.tournament_probabilities,
                   gp.reproduction_type_probabilities, gp.reproduction_probabilities, gp.num_populations,
                   device=gp.device)

    # ------------------------------------------------------------------ device
    @property
    def device(self) -> torch.device:
        if self._device is None:
            from .engine import _require_gpu
            self._device = _require_gpu(self._device_arg)  # cuda:LOCAL_RANK by default, like DeviceEngine
        return self._device

    def _device_blob(self) -> torch.Tensor:
        if self._blob is None:
            self._blob = torch.from_numpy(self._blob_host).to(self.device)
        return self._blob

    def _on_device(self, a) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(a, np.float32)) if not isinstance(a, torch.Tensor) else a
        return t.to(self.device, torch.float32).contiguous()

    def evolve(self, populations, fitness, seed: int, current_generation: int) -> torch.Tensor:
        pops, fit = self._on_device(populations), self._on_device(fitness)
        if pops.ndim != 5 or pops.shape[0] != self.num_populations or \
                tuple(pops.shape[2:]) != (self.num_trees, self.N, 4):
            raise ValueError(f"populations shape {tuple(pops.shape)} does not match the strategy")
        if fit.shape != pops.shape[:2]:
            raise ValueError(f"fitness shape {tuple(fit.shape)} does not match populations {tuple(pops.shape[:2])}")
        P, S = pops.shape[:2]
        E = self.cfg.elite_size
        pairs = (S - E) // 2
        nws = self.hip.mtgp_evolve_workspace_bytes(P, S)
        if nws < 0:
            raise ValueError("mtgp_evolve_workspace_bytes rejected the population size")
        blob = self._device_blob()
        with torch.cuda.device(self.device):
            out = torch.empty((P, E + 2 * pairs, self.num_trees, self.N, 4), dtype=torch.float32, device=self.device)
            ws = torch.empty(nws // 4, dtype=torch.int32, device=self.device)
            self.cfg.current_generation = int(current_generation)
            rc = self.hip.mtgp_evolve_device(pops.data_ptr(), fit.data_ptr(), P, S, self.num_trees, self.N,
                                             ctypes.addressof(self.cfg), blob.data_ptr(), seed & _U64,
                                             ws.data_ptr(), out.data_ptr(),
                                             torch.cuda.current_stream(self.device).cuda_stream)
        if rc < 0:
            raise ValueError(f"mtgp_evolve_device failed with code {rc}")
        return out

    def sample_population(self, pop_size: int, seed: int) -> torch.Tensor:
        blob = self._device_blob()
        with torch.cuda.device(self.device):
            out = torch.empty((self.num_populations, pop_size, self.num_trees, self.N, 4), dtype=torch.float32,
                              device=self.device)
            rc = self.hip.mtgp_sample_population_device(self.num_populations, pop_size, self.num_trees, self.N,
                                                        ctypes.addressof(self.cfg), blob.data_ptr(), seed & _U64,
                                                        out.data_ptr(),
                                                        torch.cuda.current_stream(self.device).cuda_stream)
        if rc < 0:
            raise ValueError(f"mtgp_sample_population_device failed with code {rc}")
        return out

    # --------------------------------------------------------------- host twins
    def evolve_host(self, populations, fitness, seed: int, current_generation: int) -> np.ndarray:
        """The kernels' core code on the CPU (mtgp_evolve_device_host); numpy in, numpy out."""
        pops = np.ascontiguousarray(populations, np.float32)
        fit = np.ascontiguousarray(fitness, np.float32)
        if pops.ndim != 5 or pops.shape[0] != self.num_populations or pops.shape[2:] != (self.num_trees, self.N, 4):
            raise ValueError(f"populations shape {pops.shape} does not match the strategy")
        if fit.shape != pops.shape[:2]:
            raise ValueError(f"fitness shape {fit.shape} does not match populations {pops.shape[:2]}")
        P, S = pops.shape[:2]
        pairs = (S - self.cfg.elite_size) // 2
        out = np.empty((P, self.cfg.elite_size + 2 * pairs, self.num_trees, self.N, 4), np.float32)
        self.cfg.current_generation = int(current_generation)
        rc = self.hip.mtgp_evolve_device_host(pops.ctypes.data, fit.ctypes.data, P, S, self.num_trees, self.N,
                                              ctypes.addressof(self.cfg), seed & _U64, out.ctypes.data)
        if rc < 0:
            raise ValueError("mtgp_evolve_device_host rejected its arguments")
        return out

    def sample_population_host(self, pop_size: int, seed: int) -> np.ndarray:
        out = np.empty((self.num_populations, pop_size, self.num_trees, self.N, 4), np.float32)
        rc = self.hip.mtgp_sample_population_device_host(self.num_populations, pop_size, self.num_trees, self.N,
                                                         ctypes.addressof(self.cfg), seed & _U64, out.ctypes.data)
        if rc < 0:
            raise ValueError("mtgp_sample_population_device_host rejected its arguments")
        return out
