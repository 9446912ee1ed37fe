"""overiva_amd -- MI355X (gfx950) implementation of the AuxIVA / OverIVA iteration hot path of
onolab-tmu/overiva behind the reference's own Python signatures.

    from overiva_amd import overiva, auxiva_pca
    from overiva_amd import overiva_batch      # many same-shape problems per set of launches
    from overiva_amd import ogive_batch        # the same for OGIVE, a stopping rule per problem
    from overiva_amd import overiva_batch_ragged   # problems of different frame counts in one batch
    from overiva_amd import auxiva_pca_batch   # PCA + determined AuxIVA for many rooms per call
    from overiva_amd import ilrma_batch, ilrma # ILRMA (NMF source model) for many rooms per call; the algorithm of DESIGN.md 3.9
    from overiva_amd import auxiva_iss_batch, auxiva_iss   # determined AuxIVA by rank-1 ISS updates for many rooms per call; the algorithm of DESIGN.md 3.15
    from overiva_amd import overiva_ip2_batch, overiva_ip2   # OverIVA / AuxIVA with pairwise IP2 updates for many rooms per call; the algorithm of DESIGN.md 3.17
    from overiva_amd import five_batch, five   # single-source extraction by FIVE for many rooms per call; the algorithm of DESIGN.md 3.16
    from overiva_amd import separate_batch     # audio in, audio out for many rooms, X and Y staying on the device
    from overiva_amd import bss_eval_batch, bss_eval_sources   # SDR / SIR / SAR of many rooms per call; the algorithm of DESIGN.md 3.10
    from overiva_amd import bss_eval_sets_batch, bss_eval_sets, BssEvalSets   # the same for many sets of estimates per set of references: the reference half once
    from overiva_amd import simulate_batch, rir_batch   # shoebox image-source rooms for many rooms per call; the algorithm of DESIGN.md 3.11
    from overiva_amd import sweep_batch        # geometry to SDR curves, every hand-over on the device
    from overiva_amd import standard_normal_batch   # seeded normals drawn on the device: the noise and filler of seed=...
    from overiva_amd import measure_rt60_batch, absorption_for_rt60   # decay curve and RT60 of every response; the absorption for a wanted RT60

Host code is Python (as the reference is); all arithmetic on the path runs in hand-written HIP
kernels reached through the C ABI of ``liboveriva_hip.so`` (``include/overiva_hip.h``).  There is
no CPU fallback: without the built library the calls raise ``HipLibraryMissing``.
"""
from . import _lib as _lib_mod

# The host driver of this platform shares device memory between processes through dmabuf only (RCCL, the library's own
# exchanges): the variable must be in the environment BEFORE the process's first GPU call, whatever launched the process.
_lib_mod._set_ipc_env_at_import()

from ._lib import HipError, HipLibraryMissing  # noqa: E402,F401
from .acoustics import DecayBatch, absorption_for_rt60, edc_batch, measure_rt60_batch, truncation_horizon  # noqa: E402,F401
from .auxiva_pca import auxiva_pca  # noqa: F401
from .batch import BatchPlan, DeviceBatch, RaggedBatchPlan, last_batch_info, ogive_batch, overiva_batch, overiva_batch_ragged  # noqa: F401
from .five import five, five_batch  # noqa: F401
from .ilrma import ilrma, ilrma_batch  # noqa: F401
from .ip2 import overiva_ip2, overiva_ip2_batch  # noqa: F401
from .iss import auxiva_iss, auxiva_iss_batch  # noqa: F401
from .ive import ogive  # noqa: F401
from .metrics import BssEvalSets, bss_eval_batch, bss_eval_sets, bss_eval_sets_batch, bss_eval_sources  # noqa: F401
from .pca_batch import auxiva_pca_batch  # noqa: F401
from .overiva import (get_device, get_precision, last_solver_info, overiva, release_cached_buffers, set_device,  # noqa: F401
                      set_precision)
from .plan import DeviceX, Plan  # noqa: F401
from .rng import DeviceNormal, standard_normal_batch  # noqa: F401
from .room import RoomBatch, rir_batch, simulate_batch  # noqa: F401
from .separate import BatchSTFT, separate_batch  # noqa: F401
from .sweep import SweepBatch, sweep_batch  # noqa: F401
from .sharded import BinShardedSolver, disable_bin_sharding, enable_bin_sharding, shard_bounds  # noqa: F401

__all__ = ["overiva", "separate_batch", "BatchSTFT", "DeviceBatch", "overiva_batch", "overiva_batch_ragged", "ogive_batch", "auxiva_pca_batch", "ilrma_batch", "ilrma", "auxiva_iss_batch", "auxiva_iss", "overiva_ip2_batch", "overiva_ip2", "five_batch", "five", "bss_eval_batch", "bss_eval_sources", "bss_eval_sets_batch", "bss_eval_sets", "BssEvalSets", "simulate_batch", "rir_batch", "RoomBatch", "sweep_batch", "SweepBatch", "standard_normal_batch", "DeviceNormal", "measure_rt60_batch", "edc_batch", "DecayBatch", "absorption_for_rt60", "truncation_horizon", "last_batch_info", "BatchPlan", "RaggedBatchPlan", "auxiva_pca", "ogive", "Plan", "DeviceX", "BinShardedSolver", "enable_bin_sharding", "disable_bin_sharding",
           "shard_bounds", "release_cached_buffers", "set_device", "get_device", "set_precision", "get_precision", "last_solver_info", "HipError", "HipLibraryMissing"]
