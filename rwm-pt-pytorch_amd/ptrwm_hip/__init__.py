"""ctypes binding of the C-ABI engine library (include/ptrwm.h -> lib/libptrwm_hip.so).

This is the only place Python touches the HIP engine.  torch is used for device memory and streams
only: every call passes raw ``tensor.data_ptr()`` device pointers and the current HIP stream.

There is no CPU or eager-torch fallback: if the library is missing, or a tensor is not on a ROCm
device, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import torch  # noqa: F401  (must be imported first: loads the HIP runtime the library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
# PTRWM_LIB: alternative build of the same library (A/B tuning experiments)
LIB_PATH = os.environ.get("PTRWM_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libptrwm_hip.so")

ABI_VERSION = 3
MAX_DIM = 104
MAX_TEMPS = 256

# target kinds (include/ptrwm.h)
TARGET_ROUGH_CARPET = 0
TARGET_THREE_MIXTURE = 1
TARGET_FULL_ROSENBROCK = 2
TARGET_EVEN_ROSENBROCK = 3
TARGET_HYBRID_ROSENBROCK = 4
TARGET_IID_GAMMA = 5
TARGET_IID_BETA = 6
TARGET_DIAG_GAUSSIAN = 7
TARGET_HYPERCUBE = 8
TARGET_NEAL_FUNNEL = 9
# proposal kinds
PROPOSAL_NORMAL = 0
PROPOSAL_LAPLACE = 1
PROPOSAL_UNIFORM_RADIUS = 2
# swap semantics
SWAP_EXCHANGE = 0
SWAP_REFERENCE_COPY = 1
ORDER_SEQUENTIAL = 0
ORDER_EVEN_ODD = 1

# form of the fused step kernel (ptrwm_set_kernel_form): a speed choice only, results are bit-identical
FORM_AUTO, FORM_THREAD, FORM_QUAD = 0, 1, 2

# short launches (ptrwm_set_stream_mode): the streaming form of the one-thread-per-replica kernel; same bits either way
STREAM_AUTO, STREAM_OFF, STREAM_ON = 0, 1, 2

SWAP_MODES = {"exchange": SWAP_EXCHANGE, "reference_copy": SWAP_REFERENCE_COPY}
SWAP_ORDERS = {"sequential": ORDER_SEQUENTIAL, "even_odd": ORDER_EVEN_ODD}


class PTRWMError(RuntimeError):
    """A C-ABI call returned a negative status."""

    def __init__(self, code: int, where: str):
        self.code = code
        super().__init__(f"{where}: {strerror(code)} (status {code})")


class TargetDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("dim", C.c_int32),
        ("p", C.c_float * 12),
        ("ip", C.c_int32 * 4),
        ("vec0", C.c_void_p),
        ("vec1", C.c_void_p),
    ]


class ProposalDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("inv_dim", C.c_float),
        ("temp_scale", C.c_void_p),
        ("dim_scale", C.c_void_p),
    ]


class RunArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_temps", C.c_int32),
        ("n_chains", C.c_int64),
        ("chain_offset", C.c_int64),
        ("state", C.c_void_p),
        ("logp", C.c_void_p),
        ("beta", C.c_void_p),
        ("n_accept", C.c_void_p),
        ("sq_jump", C.c_void_p),
        ("swap_accept", C.c_void_p),
        ("last_swap_ordinal", C.c_void_p),
        ("step0", C.c_int64),
        ("n_steps", C.c_int64),
        ("burn_in", C.c_int64),
        ("swap_every", C.c_int32),
        ("swap_mode", C.c_int32),
        ("swap_order", C.c_int32),
        ("swap_event_offset", C.c_int32),
        ("seed", C.c_uint64),
        ("ext_prop", C.c_void_p),
        ("ext_u", C.c_void_p),
        ("ext_swap_u", C.c_void_p),
        ("trace", C.c_void_p),
        ("trace_logp", C.c_void_p),
        ("trace_chains", C.c_int64),
        ("trace_temps", C.c_int32),
        ("trace_every", C.c_int32),
        ("trace_row0", C.c_int64),
        ("accept_flags", C.c_void_p),
        ("state_f64", C.c_int32),
        ("split_flags", C.c_int32),
        ("device_step", C.c_void_p),
    ]


_MOMENTS_FIELDS = [  # of both accumulator structs: they differ in the shapes of what the pointers point to
    ("struct_size", C.c_uint32),
    ("temps", C.c_int32),
    ("every", C.c_int32),
    ("sum", C.c_void_p),
    ("sum_sq", C.c_void_p),
    ("sum_logp", C.c_void_p),
    ("count", C.c_void_p),
]


class MomentsArgs(C.Structure):
    """ptrwm_moments_args: fp64 moment sums of the first ``temps`` temperatures (include/ptrwm.h)."""
    _fields_ = _MOMENTS_FIELDS


class ChainMomentsArgs(C.Structure):
    """ptrwm_chain_moments_args: fp64 moment sums of every chain on its own (include/ptrwm.h)."""
    _fields_ = _MOMENTS_FIELDS


class FlowArgs(C.Structure):
    """ptrwm_flow_args: the flow words of every position and the round-trip / visit counters (include/ptrwm.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_int32),
        ("walker", C.c_void_p),
        ("round_trips", C.c_void_p),
        ("n_up", C.c_void_p),
        ("n_down", C.c_void_p),
    ]


class HistArgs(C.Structure):
    """ptrwm_hist_args: pooled marginal histograms of the first ``temps`` temperatures (include/ptrwm.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("temps", C.c_int32),
        ("every", C.c_int32),
        ("n_bins", C.c_int32),
        ("lo", C.c_void_p),
        ("scale", C.c_void_p),
        ("counts", C.c_void_p),
        ("count", C.c_void_p),
    ]


HIST_MAX_BINS = 1024


class AdaptArgs(C.Structure):
    """ptrwm_adapt_args: warm-up tuning of the per-temperature proposal scale (include/ptrwm.h, csrc/adapt.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("every", C.c_int32),
        ("until", C.c_int64),
        ("target", C.c_float),
        ("gain", C.c_float),
        ("decay", C.c_float),
        ("min_scale", C.c_float),
        ("max_scale", C.c_float),
        ("defer_update", C.c_int32),
        ("temp_scale", C.c_void_p),
        ("window_accept", C.c_void_p),
        ("pooled", C.c_void_p),
        ("scale_history", C.c_void_p),
        ("accept_history", C.c_void_p),
    ]


class LadderArgs(C.Structure):
    """ptrwm_ladder_args: warm-up tuning of the temperature ladder (include/ptrwm.h, csrc/ladder.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("every", C.c_int32),
        ("probe_every", C.c_int32),
        ("until", C.c_int64),
        ("gain", C.c_float),
        ("decay", C.c_float),
        ("rescale_scales", C.c_int32),
        ("defer_update", C.c_int32),
        ("beta", C.c_void_p),
        ("temp_scale", C.c_void_p),
        ("pooled", C.c_void_p),
        ("beta_history", C.c_void_p),
        ("rate_history", C.c_void_p),
        ("skipped", C.c_void_p),
    ]


class AcfArgs(C.Structure):
    """ptrwm_acf_args: pooled lagged autocovariance of the first ``temps`` temperatures (include/ptrwm.h, csrc/acf.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("temps", C.c_int32),
        ("every", C.c_int32),
        ("max_lag", C.c_int32),
        ("ring", C.c_void_p),
        ("sxy", C.c_void_p),
        ("head", C.c_void_p),
        ("tail", C.c_void_p),
        ("pairs", C.c_void_p),
    ]


ACF_MAX_LAG = 1024


class CovArgs(C.Structure):
    """ptrwm_cov_args: pooled posterior covariance sums of the first ``temps`` temperatures (include/ptrwm.h, csrc/cov.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("temps", C.c_int32),
        ("every", C.c_int32),
        ("sxx", C.c_void_p),
        ("sx", C.c_void_p),
        ("count", C.c_void_p),
    ]


class EnergyArgs(C.Structure):
    """ptrwm_energy_args: pooled log-density sums along the ladder, per group of chains (include/ptrwm.h, csrc/energy.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("groups", C.c_int32),
        ("every", C.c_int32),
        ("ref", C.c_void_p),
        ("ref_set", C.c_void_p),
        ("count", C.c_void_p),
        ("nonfinite", C.c_void_p),
        ("s1", C.c_void_p),
        ("s2", C.c_void_p),
        ("colder", C.c_void_p),
        ("hotter", C.c_void_p),
    ]


ENERGY_MAX_GROUPS = 64


class PrecondArgs(C.Structure):
    """ptrwm_precond_args: the factor of a preconditioned Normal proposal (include/ptrwm.h, csrc/precond.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("chol", C.c_void_p),
    ]


class PrecondUpdateArgs(C.Structure):
    """ptrwm_precond_update_args: the factor learned from one warm-up window's covariance sums (include/ptrwm.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("chol", C.c_void_p),
        ("sxx", C.c_void_p),
        ("sx", C.c_void_p),
        ("count", C.c_void_p),
        ("run_xx", C.c_void_p),
        ("run_x", C.c_void_p),
        ("run_w", C.c_void_p),
        ("memory", C.c_double),
        ("jitter", C.c_double),
        ("min_count", C.c_double),
        ("windows", C.c_int64),
        ("chol_history", C.c_void_p),
        ("weight_history", C.c_void_p),
        ("skipped", C.c_void_p),
    ]


class InitArgs(C.Structure):
    """ptrwm_init_args: starting points drawn from a box, or set to a fallback point (include/ptrwm.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("per_temperature", C.c_int32),
        ("attempt", C.c_int32),
        ("lo", C.c_void_p),
        ("hi", C.c_void_p),
        ("fallback", C.c_void_p),
    ]


# every symbol include/ptrwm.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ptrwm_abi_version": (C.c_int32, []),
    "ptrwm_strerror": (C.c_char_p, [C.c_int32]),
    "ptrwm_ext_raw_per_step": (C.c_int32, [C.c_int32, C.c_int32]),
    "ptrwm_has_variant": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "ptrwm_set_kernel_form": (C.c_int32, [C.c_int32]),
    "ptrwm_set_stream_mode": (C.c_int32, [C.c_int32]),
    "ptrwm_has_stream_variant": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "ptrwm_last_launch_kind": (C.c_int32, []),
    "ptrwm_last_launch_functor": (C.c_int32, []),
    "ptrwm_has_quad_variant": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ptrwm_has_thread_variant": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "ptrwm_auto_form": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "ptrwm_auto_form_for": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "ptrwm_device_simds": (C.c_int32, [C.c_void_p]),
    "ptrwm_source_hash": (C.c_char_p, []),
    "ptrwm_form_table_source_hash": (C.c_char_p, []),
    "ptrwm_run": (C.c_int32, [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.c_void_p]),
    "ptrwm_run_with_moments": (
        C.c_int32,
        [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.POINTER(MomentsArgs), C.c_void_p]),
    "ptrwm_split_moments": (C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.POINTER(MomentsArgs), C.c_void_p]),
    "ptrwm_run_with_chain_moments": (
        C.c_int32,
        [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.POINTER(ChainMomentsArgs), C.c_void_p]),
    "ptrwm_split_chain_moments": (C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.POINTER(ChainMomentsArgs), C.c_void_p]),
    "ptrwm_run_with_diagnostics": (
        C.c_int32,
        [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.POINTER(MomentsArgs), C.POINTER(ChainMomentsArgs),
         C.POINTER(FlowArgs), C.c_void_p]),
    "ptrwm_run_with_histogram": (
        C.c_int32,
        [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.POINTER(MomentsArgs), C.POINTER(ChainMomentsArgs),
         C.POINTER(FlowArgs), C.POINTER(HistArgs), C.c_void_p]),
    "ptrwm_histogram": (C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.POINTER(HistArgs), C.c_void_p]),
    "ptrwm_run_with_adaptation": (
        C.c_int32,
        [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.POINTER(MomentsArgs), C.POINTER(ChainMomentsArgs),
         C.POINTER(FlowArgs), C.POINTER(HistArgs), C.POINTER(AdaptArgs), C.c_void_p]),
    "ptrwm_adapt_reduce": (C.c_int32, [C.POINTER(RunArgs), C.POINTER(AdaptArgs), C.c_void_p]),
    "ptrwm_adapt_update": (C.c_int32, [C.POINTER(AdaptArgs), C.c_int32, C.c_int64, C.c_void_p]),
    "ptrwm_run_with_ladder": (
        C.c_int32,
        [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.POINTER(MomentsArgs), C.POINTER(ChainMomentsArgs),
         C.POINTER(FlowArgs), C.POINTER(HistArgs), C.POINTER(AdaptArgs), C.POINTER(LadderArgs), C.c_void_p]),
    "ptrwm_ladder_probe": (C.c_int32, [C.POINTER(RunArgs), C.POINTER(LadderArgs), C.c_void_p]),
    "ptrwm_ladder_update": (C.c_int32, [C.POINTER(LadderArgs), C.c_int32, C.c_int64, C.c_void_p]),
    "ptrwm_run_with_autocorr": (
        C.c_int32,
        [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.POINTER(MomentsArgs), C.POINTER(ChainMomentsArgs),
         C.POINTER(FlowArgs), C.POINTER(HistArgs), C.POINTER(AdaptArgs), C.POINTER(LadderArgs), C.POINTER(AcfArgs), C.c_void_p]),
    "ptrwm_autocorr": (C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.POINTER(AcfArgs), C.c_void_p]),
    "ptrwm_run_with_covariance": (
        C.c_int32,
        [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.POINTER(MomentsArgs), C.POINTER(ChainMomentsArgs),
         C.POINTER(FlowArgs), C.POINTER(HistArgs), C.POINTER(AdaptArgs), C.POINTER(LadderArgs), C.POINTER(AcfArgs),
         C.POINTER(CovArgs), C.c_void_p]),
    "ptrwm_covariance": (C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.POINTER(CovArgs), C.c_void_p]),
    "ptrwm_run_with_energy": (
        C.c_int32,
        [C.POINTER(TargetDesc), C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.POINTER(MomentsArgs), C.POINTER(ChainMomentsArgs),
         C.POINTER(FlowArgs), C.POINTER(HistArgs), C.POINTER(AdaptArgs), C.POINTER(LadderArgs), C.POINTER(AcfArgs),
         C.POINTER(CovArgs), C.POINTER(EnergyArgs), C.c_void_p]),
    "ptrwm_energy": (C.c_int32, [C.POINTER(RunArgs), C.POINTER(EnergyArgs), C.c_void_p]),
    "ptrwm_swap_sweep_with_flow": (
        C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.c_int64, C.c_int32, C.POINTER(FlowArgs), C.c_void_p]),
    "ptrwm_split_accept_with_flow": (
        C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FlowArgs), C.c_void_p]),
    "ptrwm_swap_sweep": (C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.c_int64, C.c_int32, C.c_void_p]),
    "ptrwm_split_propose": (
        C.c_int32, [C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptrwm_split_accept": (
        C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptrwm_split_propose_precond": (
        C.c_int32, [C.POINTER(ProposalDesc), C.POINTER(RunArgs), C.c_int32, C.POINTER(PrecondArgs), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptrwm_precond_update": (C.c_int32, [C.POINTER(PrecondUpdateArgs), C.c_int32, C.c_int64, C.c_void_p]),
    "ptrwm_split_advance": (C.c_int32, [C.POINTER(RunArgs), C.c_void_p]),
    "ptrwm_init_states": (C.c_int32, [C.POINTER(RunArgs), C.c_int32, C.POINTER(InitArgs), C.c_void_p]),
    "ptrwm_logdensity": (C.c_int32, [C.POINTER(TargetDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ptrwm_propose": (
        C.c_int32,
        [C.POINTER(ProposalDesc), C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p],
    ),
    "ptrwm_philox_raw": (
        C.c_int32,
        [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p],
    ),
}

_lib = None


def load_library(path: Optional[str] = None):
    """Load (once) and type the engine library.  Raises if it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"HIP engine library not found at {p}. Build it first: "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C rwm-pt-pytorch_amd/csrc`. "
            "There is no CPU fallback."
        )
    lib = C.CDLL(p)
    # the version first: a library of another ABI version may lack symbols this binding types below
    lib.ptrwm_abi_version.restype, lib.ptrwm_abi_version.argtypes = SYMBOLS["ptrwm_abi_version"]
    if lib.ptrwm_abi_version() != ABI_VERSION:
        raise RuntimeError(f"ABI mismatch: library {p} is version {lib.ptrwm_abi_version()}, this binding {ABI_VERSION} "
                           "(rebuild: make -C rwm-pt-pytorch_amd/csrc)")
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    form = os.environ.get("PTRWM_KERNEL_FORM")  # tuning aid: auto | thread | quad (results are identical)
    if form:
        lib.ptrwm_set_kernel_form({"auto": FORM_AUTO, "thread": FORM_THREAD, "quad": FORM_QUAD}[form.lower()])
    smode = os.environ.get("PTRWM_STREAM")  # tuning aid: auto | off | on (results are identical)
    if smode:
        lib.ptrwm_set_stream_mode({"auto": STREAM_AUTO, "off": STREAM_OFF, "on": STREAM_ON}[smode.lower()])
    if path is None:
        _lib = lib
    return lib


def strerror(code: int) -> str:
    return load_library().ptrwm_strerror(code).decode()


def _require_device(t: torch.Tensor, name: str, dtype: torch.dtype) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: the PT-RWM engine only runs on a ROCm GPU (no CPU fallback)."
        )
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.data_ptr()


def _opt(t: Optional[torch.Tensor], name: str, dtype: torch.dtype) -> Optional[int]:
    return None if t is None else _require_device(t, name, dtype)


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class on_device:
    """Makes `device` the current HIP device around a C-ABI call and restores the previous one afterwards.

    The C ABI launches on whatever device is current (the usual HIP contract, stated in include/ptrwm.h), while the
    class API accepts `device='cuda:1'` without the caller ever calling `torch.cuda.set_device`: without this guard
    the kernel would be launched on device 0 with device-1 pointers.  A no-op (two integer compares) when the device
    is already current, so the per-step launch path stays at a few microseconds."""

    __slots__ = ("idx", "prev")

    def __init__(self, device: torch.device):
        self.idx = device.index if device.index is not None else torch.cuda.current_device()
        self.prev = self.idx

    def __enter__(self):
        self.prev = torch.cuda.current_device()
        if self.prev != self.idx:
            torch.cuda.set_device(self.idx)
        return self

    def __exit__(self, *exc):
        if self.prev != self.idx:
            torch.cuda.set_device(self.prev)
        return False


@dataclass
class Target:
    """Host-side description of a target density; tensors are kept alive by the owner."""

    kind: int
    dim: int
    p: tuple = ()
    ip: tuple = ()
    vec0: Optional[torch.Tensor] = None
    vec1: Optional[torch.Tensor] = None

    def desc(self) -> TargetDesc:
        d = TargetDesc()
        d.kind = self.kind
        d.dim = self.dim
        for i, v in enumerate(self.p):
            d.p[i] = float(v)
        for i, v in enumerate(self.ip):
            d.ip[i] = int(v)
        d.vec0 = _opt(self.vec0, "target.vec0", torch.float32)
        d.vec1 = _opt(self.vec1, "target.vec1", torch.float32)
        return d


@dataclass
class Proposal:
    kind: int
    temp_scale: torch.Tensor  # [T] float32 device
    dim_scale: Optional[torch.Tensor] = None  # [D] float32 device (Laplace)
    inv_dim: float = 0.0

    def desc(self) -> ProposalDesc:
        d = ProposalDesc()
        d.kind = self.kind
        d.inv_dim = float(self.inv_dim)
        d.temp_scale = _require_device(self.temp_scale, "proposal.temp_scale", torch.float32)
        d.dim_scale = _opt(self.dim_scale, "proposal.dim_scale", torch.float32)
        return d


def ext_raw_per_step(proposal_kind: int, dim: int) -> int:
    n = load_library().ptrwm_ext_raw_per_step(proposal_kind, dim)
    if n < 0:
        raise PTRWMError(n, "ptrwm_ext_raw_per_step")
    return n


def has_variant(target_kind: int, proposal_kind: int, dim: int) -> bool:
    return bool(load_library().ptrwm_has_variant(target_kind, proposal_kind, dim))


def has_quad_variant(target_kind: int, proposal_kind: int, dim: int, n_temps: int) -> bool:
    return bool(load_library().ptrwm_has_quad_variant(target_kind, proposal_kind, dim, n_temps))


def has_thread_variant(target_kind: int, proposal_kind: int, dim: int) -> bool:
    """Is there a one-thread-per-replica step kernel for this shape (never above dim 64)?"""
    return bool(load_library().ptrwm_has_thread_variant(target_kind, proposal_kind, dim))


def auto_form(target_kind: int, proposal_kind: int, dim: int, n_temps: int, n_chains: int) -> int:
    """The form FORM_AUTO runs for a launch of this shape on the current device (FORM_THREAD or FORM_QUAD)."""
    rc = load_library().ptrwm_auto_form(target_kind, proposal_kind, dim, n_temps, n_chains)
    if rc < 0:
        raise PTRWMError(rc, "ptrwm_auto_form")
    return rc


def auto_form_for(target_kind: int, proposal_kind: int, dim: int, n_temps: int, n_chains: int, n_simds: int) -> int:
    """The AUTO rule for a device of ``n_simds`` SIMDs (a pure function of its arguments and of the fitted table)."""
    rc = load_library().ptrwm_auto_form_for(target_kind, proposal_kind, dim, n_temps, n_chains, n_simds)
    if rc < 0:
        raise PTRWMError(rc, "ptrwm_auto_form_for")
    return rc


def device_simds(device) -> int:
    """SIMDs (compute units x 4) of ``device`` as the library sees them through the device's current stream."""
    device = torch.device(device)
    with on_device(device):
        rc = load_library().ptrwm_device_simds(_stream(device))
    if rc < 0:
        raise PTRWMError(rc, "ptrwm_device_simds")
    return rc


def source_hash() -> str:
    """sha256 of the kernel sources this library was built from (tools/source_hash.py)."""
    return load_library().ptrwm_source_hash().decode()


def form_table_source_hash() -> str:
    """Hash of the kernel sources the AUTO form table (csrc/form_table.inc) was fitted on."""
    return load_library().ptrwm_form_table_source_hash().decode()


def set_kernel_form(form: int) -> int:
    """Pin the form of the fused step kernel (FORM_AUTO / FORM_THREAD / FORM_QUAD); returns the previous setting.
    The forms are bit-identical on the same Philox stream: this changes speed only (tests and tuning)."""
    prev = load_library().ptrwm_set_kernel_form(form)
    if prev < 0:
        raise PTRWMError(prev, "ptrwm_set_kernel_form")
    return prev


LAUNCH_THREAD, LAUNCH_QUAD, LAUNCH_STREAM = 1, 2, 3


def last_launch_kind() -> int:
    """Which kernel this thread's most recent ptrwm_run enqueued (LAUNCH_THREAD / LAUNCH_QUAD / LAUNCH_STREAM)."""
    return load_library().ptrwm_last_launch_kind()


FUNCTOR_GENERAL, FUNCTOR_SPECIALISED, FUNCTOR_FOLDED = 0, 1, 2


def last_launch_functor() -> int:
    """Which functor of the target this thread's most recent ptrwm_run used (FUNCTOR_GENERAL / FUNCTOR_SPECIALISED /
    FUNCTOR_FOLDED, include/ptrwm.h)."""
    return load_library().ptrwm_last_launch_functor()


def has_stream_variant(target_kind: int, proposal_kind: int, dim: int) -> bool:
    """Does the one-thread-per-replica kernel of this shape have a streaming twin for short launches?"""
    return bool(load_library().ptrwm_has_stream_variant(target_kind, proposal_kind, dim))


def set_stream_mode(mode: int) -> int:
    """When ptrwm_run takes the streaming form of the step kernel for short launches (STREAM_AUTO / STREAM_OFF /
    STREAM_ON); returns the previous setting.  The forms give the same bits: this changes speed only."""
    prev = load_library().ptrwm_set_stream_mode(mode)
    if prev < 0:
        raise PTRWMError(prev, "ptrwm_set_stream_mode")
    return prev


class stream_mode:
    """Context manager around set_stream_mode."""

    def __init__(self, mode: int):
        self.mode = mode

    def __enter__(self):
        self.prev = set_stream_mode(self.mode)
        return self

    def __exit__(self, *exc):
        set_stream_mode(self.prev)
        return False


class kernel_form:
    """Context manager around set_kernel_form."""

    def __init__(self, form: int):
        self.form = form

    def __enter__(self):
        self.prev = set_kernel_form(self.form)
        return self

    def __exit__(self, *exc):
        set_kernel_form(self.prev)
        return False


def logdensity(target: Target, x: torch.Tensor) -> torch.Tensor:
    """log-density of every row of ``x`` ([n, dim] float32 on the GPU) -> [n] float32."""
    lib = load_library()
    if x.dim() != 2 or x.shape[1] != target.dim:
        raise ValueError(f"x must have shape [n, {target.dim}], got {tuple(x.shape)}")
    xp = _require_device(x, "x", torch.float32)
    out = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    desc = target.desc()
    with on_device(x.device):
        rc = lib.ptrwm_logdensity(C.byref(desc), xp, out.data_ptr(), x.shape[0], _stream(x.device))
    if rc != 0:
        raise PTRWMError(rc, "ptrwm_logdensity")
    return out


def propose(proposal: Proposal, dim: int, n: int, seed: int = 0, ext_raw: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Proposal increments [n, T, dim] from Philox(seed) or from external raw randoms [n, T, raw]."""
    lib = load_library()
    T = proposal.temp_scale.numel()
    dev = proposal.temp_scale.device
    desc = proposal.desc()
    if ext_raw is not None:
        if tuple(ext_raw.shape) != (n, T, ext_raw_per_step(proposal.kind, dim)):
            raise ValueError(f"ext_raw has shape {tuple(ext_raw.shape)}")
    out = torch.empty(n, T, dim, device=dev, dtype=torch.float32)
    with on_device(dev):
        rc = lib.ptrwm_propose(C.byref(desc), dim, T, n, _opt(ext_raw, "ext_raw", torch.float32), seed & (2**64 - 1),
                               out.data_ptr(), _stream(dev))
    if rc != 0:
        raise PTRWMError(rc, "ptrwm_propose")
    return out


def philox_raw(seed: int, c0: int, c1: int, c2: int, c3: int, n: int, device) -> torch.Tensor:
    """n consecutive Philox4x32-10 blocks (counter c0+i) as an int64 tensor [n, 4] of uint32 values."""
    lib = load_library()
    out = torch.empty(n, 4, device=device, dtype=torch.int32)
    if not out.is_cuda:
        raise RuntimeError("philox_raw needs a ROCm device")
    with on_device(out.device):
        rc = lib.ptrwm_philox_raw(seed, c0, c1, c2, c3, n, out.data_ptr(), _stream(out.device))
    if rc != 0:
        raise PTRWMError(rc, "ptrwm_philox_raw")
    return out.to(torch.int64) & 0xFFFFFFFF


def periodic_steps_in(a: int, b: int, period: int, burn_in: int = 0) -> int:
    """Steps with step_counter in (a, b] that are past ``burn_in`` and a multiple of ``period``: the swap events
    (swap_every), accumulated steps (every) and, with burn_in = 0, traced rows (trace_every) of the steps a .. b - 1.
    The library's rule (csrc/schedule.h periodic_steps_in), for sizing buffers and counting on the host."""
    return max(0, b // period - burn_in // period) - max(0, a // period - burn_in // period)


class RunPlan:
    """The arguments of ``ptrwm_run`` that do not change between launches of one sampler run, validated and
    marshalled once.  ``launch`` only fills in the step range, the optional trace / fixture buffers and the
    current stream, so a one-step launch costs a few microseconds of host time (the reference's per-step
    ``step()`` calling pattern stays launch-bound on the kernel, not on Python).  The plan holds references to
    its tensors, so the device pointers stay valid for as long as the plan lives."""

    def __init__(
        self,
        target: Target,
        proposal: Proposal,
        *,
        state: torch.Tensor,  # [C, T, D] float32, or float64 (state_f64 of include/ptrwm.h: the reference's dtype=float64)
        logp: torch.Tensor,  # [C, T] float32
        beta: torch.Tensor,  # [T] float32
        burn_in: int = 0,
        swap_every: int = 1,
        swap_mode: int = SWAP_EXCHANGE,
        swap_order: int = ORDER_SEQUENTIAL,
        seed: int = 0,
        chain_offset: int = 0,
        n_accept: Optional[torch.Tensor] = None,  # [C, T] int64
        sq_jump: Optional[torch.Tensor] = None,  # [C, T] float64
        swap_accept: Optional[torch.Tensor] = None,  # [C, T] int64
        last_swap_ordinal: Optional[torch.Tensor] = None,  # [C, T] int64
    ):
        self._lib = load_library()
        if isinstance(state, torch.Tensor) and state.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"state must be torch.float32 or torch.float64, got {state.dtype}")
        self.state_dtype = state.dtype if isinstance(state, torch.Tensor) else torch.float32
        if state.dim() != 3:
            raise ValueError("state must be [n_chains, n_temps, dim]")
        Cn, T, D = state.shape
        if target is not None and D != target.dim:
            raise ValueError(f"state dim {D} != target dim {target.dim}")
        if tuple(logp.shape) != (Cn, T) or beta.numel() != T or proposal.temp_scale.numel() != T:
            raise ValueError("logp/beta/temp_scale shapes do not match state")
        self.shape = (Cn, T, D)
        self.proposal_kind = proposal.kind
        self.device = state.device
        for name, t in (("logp", logp), ("beta", beta), ("temp_scale", proposal.temp_scale)):
            if t.device != self.device:
                raise ValueError(f"{name} is on {t.device}, state on {self.device}: all tensors of a run live on one GPU")
        a = RunArgs()
        a.struct_size = C.sizeof(RunArgs)
        a.n_temps = T
        a.n_chains = Cn
        a.chain_offset = chain_offset
        a.state = _require_device(state, "state", self.state_dtype)
        a.state_f64 = 1 if self.state_dtype == torch.float64 else 0
        a.logp = _require_device(logp, "logp", torch.float32)
        a.beta = _require_device(beta, "beta", torch.float32)
        for name, t, dt in (
            ("n_accept", n_accept, torch.int64),
            ("sq_jump", sq_jump, torch.float64),
            ("swap_accept", swap_accept, torch.int64),
            ("last_swap_ordinal", last_swap_ordinal, torch.int64),
        ):
            if t is not None and tuple(t.shape) != (Cn, T):
                raise ValueError(f"{name} must have shape [{Cn}, {T}]")
            setattr(a, name, _opt(t, name, dt))
        a.burn_in = burn_in
        a.swap_every = swap_every
        a.swap_mode = swap_mode
        a.swap_order = swap_order
        a.seed = seed & (2**64 - 1)
        self._a = a
        # target None: a plan for split steps only (the caller evaluates the density, see split_propose)
        self._t = target.desc() if target is not None else None
        self._p = proposal.desc()
        self._refs = (self._t, self._p, C.byref(self._t) if target is not None else None, C.byref(self._p), C.byref(a))
        self._keep = (target, proposal, state, logp, beta, n_accept, sq_jump, swap_accept, last_swap_ordinal)
        self._plain = True  # no per-launch buffers set in _a
        self._last_trace = (None, None, None)  # (trace, trace_logp, trace_every) marshalled into _a by the last launch
        self._guard = on_device(self.device)  # (after the checks above: they reject CPU tensors first)
        self._mom = None  # the accumulator, pooled or per chain: (kind of _MOMENT_KINDS, struct, byref, tensors)
        self._flow = None  # replica flow: (struct, byref, tensors)
        self._hist = None  # pooled marginal histograms: (struct, byref, tensors)
        self._adapt = None  # warm-up tuning of the proposal scale: (struct, byref, tensors)
        self._ladder = None  # warm-up tuning of the temperature ladder: (struct, byref, tensors)
        self._acf = None  # pooled lagged autocovariance: (struct, byref, tensors)
        self._cov = None  # pooled posterior covariance: (struct, byref, tensors)
        self._energy = None  # pooled log-density sums along the ladder: (struct, byref, tensors)
        self._precond = None  # preconditioned proposals: (struct, byref, tensors)
        self._precond_update = None  # warm-up tuning of the factor, the update: (struct, byref, tensors)
        self._precond_probe = None  # ... and its probe, a covariance block of temperature 0: (struct, byref, tensors)
        self._warm_saved = None  # split_warmup: the run arguments it has set aside while on

    # kind of accumulator -> (words of its messages, struct, entry point of launch(), entry point of split_moments())
    _MOMENT_KINDS = {"pooled": ("moments", MomentsArgs, "ptrwm_run_with_moments", "ptrwm_split_moments"),
                     "chain": ("chain moments", ChainMomentsArgs, "ptrwm_run_with_chain_moments", "ptrwm_split_chain_moments")}

    # launch(): the first entry point that takes _flow, _hist, _adapt, _ladder, _acf, _cov, _energy - in this order - and all before it
    _RUN_WITH = ("ptrwm_run_with_diagnostics", "ptrwm_run_with_histogram", "ptrwm_run_with_adaptation", "ptrwm_run_with_ladder",
                 "ptrwm_run_with_autocorr", "ptrwm_run_with_covariance", "ptrwm_run_with_energy")

    def _bind_moments(self, kind, lead, sum, sum_sq, sum_logp, count, every) -> None:
        """The one accumulator of the plan: ``sum`` / ``sum_sq`` are [*lead, temps, dim], ``sum_logp`` [*lead, temps],
        ``count`` [temps].  ``sum`` None switches an accumulator of this kind off; anything else replaces what was set."""
        if sum is None:
            if self._mom is not None and self._mom[0] == kind:
                self._mom = None
            return
        what, struct = self._MOMENT_KINDS[kind][:2]
        T, D = self.shape[1:]

        def fmt(*shape):
            return "[" + ", ".join(str(n) for n in lead + shape) + "]"

        if sum.dim() != len(lead) + 2 or tuple(sum.shape[:-2]) != lead or sum.shape[-1] != D or not 1 <= sum.shape[-2] <= T:
            raise ValueError(f"{what} sum must be {fmt('temps', D)} with 1 <= temps <= {T}")
        temps = sum.shape[-2]
        if sum_sq is None or tuple(sum_sq.shape) != lead + (temps, D):
            raise ValueError(f"{what} sum_sq must be {fmt(temps, D)}")
        if sum_logp is not None and tuple(sum_logp.shape) != lead + (temps,):
            raise ValueError(f"{what} sum_logp must be {fmt(temps)}")
        if count is not None and tuple(count.shape) != (temps,):
            raise ValueError(f"{what} count must be [{temps}]")
        if int(every) < 1:
            raise ValueError(f"{what} every must be >= 1")
        for name, t in (("sum", sum), ("sum_sq", sum_sq), ("sum_logp", sum_logp), ("count", count)):
            if t is not None and t.device != self.device:
                raise ValueError(f"{what} {name} is on {t.device}, state on {self.device}")
        m = struct()
        m.struct_size = C.sizeof(struct)
        m.temps = temps
        m.every = int(every)
        m.sum = _require_device(sum, f"{what} sum", torch.float64)
        m.sum_sq = _require_device(sum_sq, f"{what} sum_sq", torch.float64)
        m.sum_logp = _opt(sum_logp, f"{what} sum_logp", torch.float64)
        m.count = _opt(count, f"{what} count", torch.int64)
        self._mom = (kind, m, C.byref(m), (sum, sum_sq, sum_logp, count))

    def set_moments(self, sum: Optional[torch.Tensor], sum_sq: Optional[torch.Tensor] = None, *,
                    sum_logp: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                    every: int = 1) -> None:
        """Accumulate posterior moments (include/ptrwm.h ptrwm_moments_args) in every following ``launch`` and
        ``split_moments``: ``sum`` / ``sum_sq`` [temps, dim] float64, ``sum_logp`` [temps] float64 and ``count`` [temps]
        int64 (both optional), all on the run's device and added to (+=).  ``temps`` (the first temperatures covered) is
        the first extent of ``sum``.  A plan holds ONE accumulator, pooled or per chain: this replaces whichever was set.
        ``set_moments(None)`` switches pooled moments off."""
        self._bind_moments("pooled", (), sum, sum_sq, sum_logp, count, every)

    def set_chain_moments(self, sum: Optional[torch.Tensor], sum_sq: Optional[torch.Tensor] = None, *,
                          sum_logp: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                          every: int = 1) -> None:
        """Accumulate the moments of every chain on its own (include/ptrwm.h ptrwm_chain_moments_args) in every following
        ``launch`` and ``split_moments``: ``sum`` / ``sum_sq`` [n_chains, temps, dim] float64, ``sum_logp``
        [n_chains, temps] float64 and ``count`` [temps] int64 (both optional), all on the run's device and added to (+=).
        A plan holds ONE accumulator, pooled or per chain: this replaces whichever was set.
        ``set_chain_moments(None)`` switches per-chain moments off."""
        self._bind_moments("chain", (self.shape[0],), sum, sum_sq, sum_logp, count, every)

    def set_flow(self, walker: Optional[torch.Tensor], round_trips: Optional[torch.Tensor] = None,
                 n_up: Optional[torch.Tensor] = None, n_down: Optional[torch.Tensor] = None) -> None:
        """Track replica flow (include/ptrwm.h ptrwm_flow_args) in every following ``launch``, ``split_accept`` and
        ``swap_sweep``: ``walker`` [n_chains, n_temps] int32 flow words (the caller starts them at ``arange(n_temps)`` per
        ladder), ``round_trips`` (by walker id), ``n_up`` and ``n_down`` (by temperature) [n_chains, n_temps] int64, each
        optional, all on the run's device and added to (+=).  ``set_flow(None)`` switches flow off."""
        if walker is None:
            self._flow = None
            return
        Cn, T, _ = self.shape
        if T < 2:
            raise ValueError("replica flow needs a ladder of at least two temperatures")
        for name, t in (("walker", walker), ("round_trips", round_trips), ("n_up", n_up), ("n_down", n_down)):
            if t is not None and (tuple(t.shape) != (Cn, T) or t.device != self.device):
                raise ValueError(f"flow {name} must be a [{Cn}, {T}] tensor on {self.device}")
        f = FlowArgs()
        f.struct_size = C.sizeof(FlowArgs)
        f.walker = _require_device(walker, "flow walker", torch.int32)
        f.round_trips = _opt(round_trips, "flow round_trips", torch.int64)
        f.n_up = _opt(n_up, "flow n_up", torch.int64)
        f.n_down = _opt(n_down, "flow n_down", torch.int64)
        self._flow = (f, C.byref(f), (walker, round_trips, n_up, n_down))

    def _bind_block(self, what: str, struct, scalars: dict, pointers) -> tuple:
        """(struct, byref, tensors) of a bound block - a snapshot accumulator, a warm-up tuning - whose messages start with
        `what`: `scalars` go into their fields as they are, every tensor of `pointers` - (field, tensor or None, dtype), shapes
        already checked - sits on the plan's device and is marshalled into its field."""
        for name, t, _ in pointers:
            if t is not None and t.device != self.device:
                raise ValueError(f"{what} {name} is on {t.device}, state on {self.device}")
        b = struct()
        b.struct_size = C.sizeof(struct)
        for name, v in scalars.items():
            setattr(b, name, v)
        for name, t, dtype in pointers:
            setattr(b, name, _opt(t, f"{what} {name}", dtype))
        return (b, C.byref(b), tuple(t for _, t, _ in pointers))

    def _split_call(self, name: str, block, step: int) -> None:
        """A stand-alone accumulator call behind the split step ``step``: ``name``(args, dim, block, stream)"""
        self._a.step0 = step
        with self._guard:
            rc = getattr(self._lib, name)(self._refs[4], self.shape[2], block, _stream(self.device))
        if rc != 0:
            raise PTRWMError(rc, name)

    def split_snapshots(self, step: int) -> None:
        """Every accumulator bound, behind the split step ``step`` just performed: moments, histogram, autocovariance,
        covariance, log-density sums, in this order (the library skips the steps that are not due)."""
        self.split_moments(step)
        self.split_histogram(step)
        self.split_autocorr(step)
        self.split_covariance(step)
        self.split_energy(step)

    def set_histogram(self, counts: Optional[torch.Tensor], lo: Optional[torch.Tensor] = None,
                      scale: Optional[torch.Tensor] = None, *, n_bins: int = 0, temps: int = 0, every: int = 1,
                      count: Optional[torch.Tensor] = None) -> None:
        """Accumulate pooled marginal histograms (include/ptrwm.h ptrwm_hist_args) in every following ``launch`` and
        ``split_histogram``: ``counts`` [temps, dim, n_bins + 2] int64 (bin 0 underflow, bin n_bins + 1 overflow), ``lo`` and
        ``scale`` = n_bins / (hi - lo) [dim] float32, ``count`` [temps] int64 (optional), all on the run's device; counts and
        count are added to (+=).  ``launch`` then ends a kernel launch at every due step and enqueues the snapshot kernel
        behind it.  ``set_histogram(None)`` switches histograms off."""
        if counts is None:
            self._hist = None
            return
        T, D = self.shape[1:]
        n_bins, temps, every = int(n_bins), int(temps), int(every)
        if not 1 <= n_bins <= HIST_MAX_BINS:
            raise ValueError(f"histogram n_bins must be in 1..{HIST_MAX_BINS}, got {n_bins}")
        if not 1 <= temps <= T:
            raise ValueError(f"histogram temps must be in 1..{T}, got {temps}")
        if every < 1:
            raise ValueError("histogram every must be >= 1")
        if tuple(counts.shape) != (temps, D, n_bins + 2):
            raise ValueError(f"histogram counts must be [{temps}, {D}, {n_bins + 2}]")
        if count is not None and tuple(count.shape) != (temps,):
            raise ValueError(f"histogram count must be [{temps}]")
        for name, t in (("lo", lo), ("scale", scale)):
            if t is None or tuple(t.shape) != (D,):
                raise ValueError(f"histogram {name} must be a [{D}] float32 tensor")
        self._hist = self._bind_block("histogram", HistArgs, dict(temps=temps, every=every, n_bins=n_bins),
                                      (("counts", counts, torch.int64), ("lo", lo, torch.float32), ("scale", scale, torch.float32),
                                       ("count", count, torch.int64)))

    def set_autocorr(self, ring: Optional[torch.Tensor], sxy: Optional[torch.Tensor] = None, head: Optional[torch.Tensor] = None,
                     tail: Optional[torch.Tensor] = None, pairs: Optional[torch.Tensor] = None, *, every: int = 1) -> None:
        """Accumulate the pooled lagged autocovariance (include/ptrwm.h ptrwm_acf_args) in every following ``launch`` and
        ``split_autocorr``: ``ring`` [max_lag, n_chains, temps, dim] of the state's dtype (scratch: the last ``max_lag``
        snapshots), ``sxy`` / ``head`` / ``tail`` [temps, max_lag + 1, dim] float64 and ``pairs`` [max_lag + 1] int64, all on the
        run's device; the sums are added to (+=).  ``temps`` and ``max_lag`` are read off ``ring``.  ``launch`` then ends a
        kernel launch at every due step and enqueues the snapshot kernel behind it.  Every due step must be snapshotted, in
        order (csrc/acf.h).  ``set_autocorr(None)`` switches it off."""
        if ring is None:
            self._acf = None
            return
        Cn, T, D = self.shape
        if ring.dim() != 4 or ring.shape[1] != Cn or ring.shape[3] != D:
            raise ValueError(f"autocorr ring must be [max_lag, {Cn}, temps, {D}]")
        max_lag, temps, every = int(ring.shape[0]), int(ring.shape[2]), int(every)
        if not 1 <= max_lag <= ACF_MAX_LAG:
            raise ValueError(f"autocorr max_lag must be in 1..{ACF_MAX_LAG}, got {max_lag}")
        if not 1 <= temps <= T:
            raise ValueError(f"autocorr temps must be in 1..{T}, got {temps}")
        if every < 1:
            raise ValueError("autocorr every must be >= 1")
        for name, t in (("sxy", sxy), ("head", head), ("tail", tail)):
            if t is None or tuple(t.shape) != (temps, max_lag + 1, D):
                raise ValueError(f"autocorr {name} must be [{temps}, {max_lag + 1}, {D}]")
        if pairs is None or tuple(pairs.shape) != (max_lag + 1,):
            raise ValueError(f"autocorr pairs must be [{max_lag + 1}]")
        self._acf = self._bind_block("autocorr", AcfArgs, dict(temps=temps, every=every, max_lag=max_lag),
                                     (("ring", ring, self.state_dtype), ("sxy", sxy, torch.float64), ("head", head, torch.float64),
                                      ("tail", tail, torch.float64), ("pairs", pairs, torch.int64)))

    def split_autocorr(self, step: int) -> None:
        """Autocovariance snapshot of the state after the split step ``step`` just performed (ptrwm_autocorr; device-step mode:
        counter + step - decided on the device, so the call can sit in a captured block).  Enqueue after ``split_accept``
        (and ``split_histogram``), behind EVERY step: the library skips the steps that are not due.  No-op without an
        accumulator."""
        if self._acf is not None:
            self._split_call("ptrwm_autocorr", self._acf[1], step)

    def set_covariance(self, sxx: Optional[torch.Tensor], sx: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                       *, every: int = 1) -> None:
        """Accumulate the pooled posterior covariance sums (include/ptrwm.h ptrwm_cov_args) in every following ``launch`` and
        ``split_covariance``: ``sxx`` [temps, dim, dim] float64 (only the lower triangle, j <= i, is added to), ``sx``
        [temps, dim] float64 and ``count`` [1] int64, all on the run's device; the sums are added to (+=).  ``temps`` is read
        off ``sxx``.  ``launch`` then ends a kernel launch at every due step and enqueues the snapshot kernel behind it.
        ``set_covariance(None)`` switches it off."""
        if sxx is None:
            self._cov = None
            return
        Cn, T, D = self.shape
        if sxx.dim() != 3 or sxx.shape[1] != D or sxx.shape[2] != D:
            raise ValueError(f"covariance sxx must be [temps, {D}, {D}]")
        temps, every = int(sxx.shape[0]), int(every)
        if not 1 <= temps <= T:
            raise ValueError(f"covariance temps must be in 1..{T}, got {temps}")
        if every < 1:
            raise ValueError("covariance every must be >= 1")
        if sx is None or tuple(sx.shape) != (temps, D):
            raise ValueError(f"covariance sx must be [{temps}, {D}]")
        if count is None or tuple(count.shape) != (1,):
            raise ValueError("covariance count must be [1]")
        self._cov = self._bind_block("covariance", CovArgs, dict(temps=temps, every=every),
                                     (("sxx", sxx, torch.float64), ("sx", sx, torch.float64), ("count", count, torch.int64)))

    def split_covariance(self, step: int) -> None:
        """Covariance snapshot of the state after the split step ``step`` just performed (ptrwm_covariance; device-step mode:
        counter + step - decided on the device, so the call can sit in a captured block).  Enqueue after ``split_accept``
        (and ``split_histogram`` / ``split_autocorr``), behind every step: the library skips the steps that are not due.
        No-op without an accumulator."""
        if self._cov is not None:
            self._split_call("ptrwm_covariance", self._cov[1], step)

    def set_energy(self, count: Optional[torch.Tensor], s1: Optional[torch.Tensor] = None, s2: Optional[torch.Tensor] = None,
                   colder: Optional[torch.Tensor] = None, hotter: Optional[torch.Tensor] = None, *,
                   ref: Optional[torch.Tensor] = None, ref_set: Optional[torch.Tensor] = None,
                   nonfinite: Optional[torch.Tensor] = None, every: int = 1) -> None:
        """Accumulate the pooled log-density sums along the ladder (include/ptrwm.h ptrwm_energy_args) in every following
        ``launch`` and ``split_energy``: ``count`` [groups, n_temps] int64, ``s1`` / ``s2`` / ``colder`` / ``hotter``
        [groups, n_temps] float64 (the last two may be None with one temperature), ``ref`` [n_temps] float64 and ``ref_set``
        [1] int32 (0: the first due snapshot sets ``ref``; pre-set to pin it), ``nonfinite`` [1] int64 (optional), all on the
        run's device; the sums are added to (+=).  ``groups`` (1..64) is read off ``count``.  ``launch`` then ends a kernel
        launch at every due step and enqueues the two kernels behind it.  ``set_energy(None)`` switches it off."""
        if count is None:
            self._energy = None
            return
        T = self.shape[1]
        if count.dim() != 2 or count.shape[1] != T:
            raise ValueError(f"energy count must be [groups, {T}]")
        groups, every = int(count.shape[0]), int(every)
        if not 1 <= groups <= ENERGY_MAX_GROUPS:
            raise ValueError(f"energy groups must be in 1..{ENERGY_MAX_GROUPS}, got {groups}")
        if every < 1:
            raise ValueError("energy every must be >= 1")
        for name, t in (("s1", s1), ("s2", s2), ("colder", colder), ("hotter", hotter)):
            if t is None and name in ("colder", "hotter") and T == 1:
                continue
            if t is None or tuple(t.shape) != (groups, T):
                raise ValueError(f"energy {name} must be [{groups}, {T}]")
        if ref is None or tuple(ref.shape) != (T,):
            raise ValueError(f"energy ref must be [{T}]")
        if ref_set is None or tuple(ref_set.shape) != (1,):
            raise ValueError("energy ref_set must be [1]")
        if nonfinite is not None and tuple(nonfinite.shape) != (1,):
            raise ValueError("energy nonfinite must be [1]")
        self._energy = self._bind_block("energy", EnergyArgs, dict(groups=groups, every=every),
                                        (("ref", ref, torch.float64), ("ref_set", ref_set, torch.int32), ("count", count, torch.int64),
                                         ("nonfinite", nonfinite, torch.int64), ("s1", s1, torch.float64), ("s2", s2, torch.float64),
                                         ("colder", colder, torch.float64), ("hotter", hotter, torch.float64)))

    def split_energy(self, step: int) -> None:
        """Log-density sums of the state after the split step ``step`` just performed (ptrwm_energy, which takes no dim;
        device-step mode: counter + step - decided on the device, as is whether ``ref`` is still to be set, so the call can sit
        in a captured block).  Enqueue after ``split_accept``, behind every step: the library skips the steps that are not due.
        No-op without an accumulator."""
        if self._energy is not None:
            self._a.step0 = step
            with self._guard:
                rc = self._lib.ptrwm_energy(self._refs[4], self._energy[1], _stream(self.device))
            if rc != 0:
                raise PTRWMError(rc, "ptrwm_energy")

    def _tuning_windows(self, what: str, every, until) -> tuple:
        """every, until and K = until // every of a warm-up tuning (`what` starts its messages), checked against the plan"""
        every, until = int(every), int(until)
        if every < 1:
            raise ValueError(f"{what} every must be >= 1")
        if not 0 <= until <= self._a.burn_in:
            raise ValueError(f"{what} until must be in 0..burn_in = {self._a.burn_in}, got {until}")
        return every, until, until // every

    def _tuning_tensors(self, what: str, tensors) -> list:
        """The shape check in front of _bind_block: (field, tensor, dtype, shape, required) of a warm-up tuning - every tensor
        given, and every required one, is there in its shape (one message, which names the device too) - as _bind_block's
        `pointers`"""
        for name, t, _, shape, required in tensors:
            if (t is None and required) or (t is not None and (tuple(t.shape) != shape or t.device != self.device)):
                raise ValueError(f"{what} {name} must be a {list(shape)} tensor on {self.device}")
        return [spec[:3] for spec in tensors]

    def _tuning_call(self, name: str, bound, missing: str, window: Optional[int] = None, extent: int = 1) -> None:
        """A stand-alone kernel of a warm-up tuning, ptrwm_<name>: the ones between launches take the run's arguments, the
        updates (`window` given) an extent of the plan's shape - n_temps, or with `extent` = 2 dim - and the window"""
        if bound is None:
            raise RuntimeError(f"{name}: no {missing}")
        args = (self._refs[4], bound[1]) if window is None else (bound[1], self.shape[extent], int(window))
        with self._guard:
            rc = getattr(self._lib, "ptrwm_" + name)(*args, _stream(self.device))
        if rc != 0:
            raise PTRWMError(rc, "ptrwm_" + name)

    def set_adaptation(self, window_accept: Optional[torch.Tensor], pooled: Optional[torch.Tensor] = None, *, every: int = 50,
                       until: int = 0, target: float = 0.234, gain: float = 3.0, decay: float = 0.5,
                       min_scale: float = 1e-30, max_scale: float = 1e30, defer_update: bool = False,
                       scale_history: Optional[torch.Tensor] = None, accept_history: Optional[torch.Tensor] = None) -> None:
        """Tune the proposal scale of every temperature during burn-in (include/ptrwm.h ptrwm_adapt_args) in every following
        ``launch``: the plan's own ``proposal.temp_scale`` is rewritten in place after every window of ``every`` steps that
        ends at or before ``until`` (<= burn_in).  ``window_accept`` [n_chains, n_temps] int64 and ``pooled`` [n_temps + 1]
        int64 are scratch, zero before the run; ``scale_history`` [K + 1, n_temps] float32 and ``accept_history``
        [K, n_temps] int64 (K = until // every) are optional records.  ``defer_update``: ``launch`` stops at window ends and
        the caller all-reduces ``pooled`` and calls ``adapt_update``.  ``set_adaptation(None)`` switches it off."""
        if window_accept is None:
            self._adapt = None
            return
        Cn, T, _ = self.shape
        every, until, K = self._tuning_windows("adaptation", every, until)
        pointers = self._tuning_tensors("adaptation", (
            ("window_accept", window_accept, torch.int64, (Cn, T), True), ("pooled", pooled, torch.int64, (T + 1,), True),
            ("scale_history", scale_history, torch.float32, (K + 1, T), False),
            ("accept_history", accept_history, torch.int64, (K, T), False)))
        # (temp_scale: the plan's own tensor, checked and marshalled with the proposal)
        self._adapt = self._bind_block("adaptation", AdaptArgs, dict(
            every=every, until=until, target=float(target), gain=float(gain), decay=float(decay), min_scale=float(min_scale),
            max_scale=float(max_scale), defer_update=1 if defer_update else 0, temp_scale=self._p.temp_scale), pointers)

    def adapt_reduce(self) -> None:
        """The end of an adapting window, stand-alone (ptrwm_adapt_reduce): ``window_accept`` summed over chains into
        ``pooled``, the scratch left zero.  ``launch`` does this itself; split steps and tests call it."""
        self._tuning_call("adapt_reduce", self._adapt, "adaptation set (set_adaptation)")

    def adapt_update(self, window: int) -> None:
        """The scale update of window ``window`` from ``pooled`` (ptrwm_adapt_update); ``pooled`` is left zero."""
        self._tuning_call("adapt_update", self._adapt, "adaptation set (set_adaptation)", window)

    def set_ladder(self, pooled: Optional[torch.Tensor], *, every: int = 100, probe_every: Optional[int] = None, until: int = 0,
                   gain: float = 2.0, decay: float = 0.5, rescale_scales: bool = True, defer_update: bool = False,
                   beta_history: Optional[torch.Tensor] = None, rate_history: Optional[torch.Tensor] = None,
                   skipped: Optional[torch.Tensor] = None) -> None:
        """Tune the temperature ladder during burn-in (include/ptrwm.h ptrwm_ladder_args) in every following ``launch``: the
        plan's own ``beta`` (and, with ``rescale_scales``, ``proposal.temp_scale``) is rewritten in place after every window of
        ``every`` steps that ends at or before ``until`` (<= burn_in), from probes behind every ``probe_every``-th step
        (default: one per window).  ``pooled`` [n_temps] int64 is scratch, zero before the run; ``beta_history``
        [K + 1, n_temps] float32, ``rate_history`` [K, n_temps] int64 (K = until // every) and ``skipped`` [1] int64 are
        optional records.  ``defer_update``: ``launch`` stops at window ends and the caller all-reduces ``pooled`` and calls
        ``ladder_update``.  The library cannot read the ladder before it enqueues: that ``beta`` is positive and strictly
        decreasing is checked here, on the host (one read).  ``set_ladder(None)`` switches it off."""
        if pooled is None:
            self._ladder = None
            return
        _, T, _ = self.shape
        if T < 3:
            raise ValueError(f"the ladder's tuning moves interior temperatures: it needs at least 3, got {T}")
        every, until, K = self._tuning_windows("ladder", every, until)
        probe_every = every if probe_every is None else int(probe_every)
        if probe_every < 1 or every % probe_every != 0:
            raise ValueError(f"ladder probe_every must be >= 1 and divide every = {every}, got {probe_every}")
        pointers = self._tuning_tensors("ladder", (
            ("pooled", pooled, torch.int64, (T,), True), ("beta_history", beta_history, torch.float32, (K + 1, T), False),
            ("rate_history", rate_history, torch.int64, (K, T), False), ("skipped", skipped, torch.int64, (1,), False)))
        b = self._keep[4].detach().cpu().numpy()
        if not (b > 0).all() or not (b[:-1] > b[1:]).all():
            raise ValueError("the ladder's tuning needs a positive, strictly decreasing beta ladder")
        # (beta, temp_scale: the plan's own tensors, checked and marshalled with the run's arguments and the proposal)
        self._ladder = self._bind_block("ladder", LadderArgs, dict(
            every=every, probe_every=probe_every, until=until, gain=float(gain), decay=float(decay),
            rescale_scales=1 if rescale_scales else 0, defer_update=1 if defer_update else 0, beta=self._a.beta,
            temp_scale=self._p.temp_scale), pointers)

    def ladder_probe(self) -> None:
        """One probe of the current log-densities, stand-alone (ptrwm_ladder_probe): every pair's quantised swap probability
        added to ``pooled``.  ``launch`` does this itself behind every probe step; split steps and tests call it."""
        self._tuning_call("ladder_probe", self._ladder, "ladder tuning set (set_ladder)")

    def ladder_update(self, window: int) -> None:
        """The ladder update of window ``window`` from ``pooled`` (ptrwm_ladder_update); ``pooled`` is left zero."""
        self._tuning_call("ladder_update", self._ladder, "ladder tuning set (set_ladder)", window)

    def split_warmup(self, on: bool) -> None:
        """Split steps inside an adapting window (include/ptrwm.h, the split-step recipe): while on, split_accept counts every
        step's acceptances into the adaptation's ``window_accept``, adds no squared jump and performs no swap event
        (burn_in = 0, swap_every = INT32_MAX, sq_jump = NULL); off restores the plan's own arguments."""
        a = self._a
        if on:
            if self._adapt is None:
                raise RuntimeError("split_warmup: no adaptation set (set_adaptation)")
            if self._warm_saved is None:
                self._warm_saved = (a.burn_in, a.swap_every, a.n_accept, a.sq_jump)
            a.burn_in, a.swap_every, a.n_accept, a.sq_jump = 0, 2**31 - 1, self._adapt[0].window_accept, None
        elif self._warm_saved is not None:
            a.burn_in, a.swap_every, a.n_accept, a.sq_jump = self._warm_saved
            self._warm_saved = None

    def split_histogram(self, step: int) -> None:
        """Histogram snapshot of the state after the split step ``step`` just performed (ptrwm_histogram; device-step mode:
        counter + step - decided on the device, so the call can sit in a captured block).  Enqueue after ``split_accept``.
        No-op without a histogram."""
        if self._hist is not None:
            self._split_call("ptrwm_histogram", self._hist[1], step)

    def init_states(self, lo: torch.Tensor, hi: torch.Tensor, *, attempt: int = 0, per_temperature: bool = False,
                    fallback: Optional[torch.Tensor] = None) -> None:
        """Starting points (ptrwm_init_states): every row of ``state`` drawn uniformly from the box ``lo``..``hi`` ([dim]
        float32 on the run's device) on Philox stream 3, keyed by the run's seed and the global chain id.  ``attempt`` > 0
        rewrites only the rows whose ``logp`` is not finite, with a fresh draw, or with ``fallback`` ([dim] float32) when
        that is given; ``per_temperature``: every temperature of a ladder draws its own point.  Enqueues only; the caller
        evaluates ``logp`` afterwards."""
        D = self.shape[2]
        for name, t in (("lo", lo), ("hi", hi), ("fallback", fallback)):
            if t is not None and (tuple(t.shape) != (D,) or t.device != self.device):
                raise ValueError(f"init_states: {name} must be a [{D}] float32 tensor on {self.device}")
        i = InitArgs()
        i.struct_size = C.sizeof(InitArgs)
        i.per_temperature = 1 if per_temperature else 0
        i.attempt = int(attempt)
        i.lo = _require_device(lo, "lo", torch.float32)
        i.hi = _require_device(hi, "hi", torch.float32)
        i.fallback = _opt(fallback, "fallback", torch.float32)
        with self._guard:
            rc = self._lib.ptrwm_init_states(self._refs[4], D, C.byref(i), _stream(self.device))
        if rc != 0:
            raise PTRWMError(rc, "ptrwm_init_states")

    def split_moments(self, step: int) -> None:
        """Moments of the split step ``step`` just performed, pooled or per chain as set (ptrwm_split_moments /
        ptrwm_split_chain_moments; device-step mode: counter + step).  Enqueue after ``split_accept``.  No-op without an
        accumulator."""
        if self._mom is not None:
            self._split_call(self._MOMENT_KINDS[self._mom[0]][3], self._mom[2], step)

    def launch(
        self,
        step0: int,
        n_steps: int,
        *,
        ext_prop: Optional[torch.Tensor] = None,
        ext_u: Optional[torch.Tensor] = None,
        ext_swap_u: Optional[torch.Tensor] = None,
        trace: Optional[torch.Tensor] = None,  # [rows, trace_chains, trace_temps, D]
        trace_logp: Optional[torch.Tensor] = None,
        trace_row0: int = 0,
        trace_every: int = 1,
        accept_flags: Optional[torch.Tensor] = None,  # [n_steps, C, T] uint8
        swap_event_offset: int = 0,  # stand-alone sweeps (swap_sweep) performed before this launch
    ) -> None:
        """Enqueue ``n_steps`` fused MH(+swap) steps, starting at global step ``step0``, on the current stream."""
        if self._t is None:
            raise RuntimeError("this plan has no target description: use split_propose / split_accept")
        a = self._a
        if a.device_step:
            raise RuntimeError("device-step mode is for split steps only: set_device_step(None) before launch()")
        a.step0 = step0
        a.n_steps = n_steps
        a.swap_event_offset = swap_event_offset
        plain = (ext_prop is None and ext_u is None and ext_swap_u is None and trace is None and trace_logp is None
                 and accept_flags is None)
        # trace-only launches into the SAME buffers as the previous launch (the reference's step()-at-a-time pattern with
        # chain storage): only the row offset moves - skip re-marshalling (a dozen ctypes field stores, ~4 us)
        same_trace = (trace is not None and trace is self._last_trace[0] and trace_logp is self._last_trace[1]
                      and trace_every == self._last_trace[2] and ext_prop is None and ext_u is None and ext_swap_u is None
                      and accept_flags is None)
        if same_trace:
            te = a.trace_every
            if trace.shape[0] < trace_row0 + periodic_steps_in(step0, step0 + n_steps, te):
                raise ValueError("trace must be [rows >= trace_row0 + traced steps, trace_chains, trace_temps, dim]")
            a.trace_row0 = trace_row0
        elif not (plain and self._plain):
            self._last_trace = (None, None, None)
            Cn, T, D = self.shape
            a.ext_prop = _opt(ext_prop, "ext_prop", self.state_dtype)  # (the state's dtype: double normals for double states)
            a.ext_u = _opt(ext_u, "ext_u", torch.float32)
            a.ext_swap_u = _opt(ext_swap_u, "ext_swap_u", torch.float32)
            if ext_prop is not None:
                raw = ext_raw_per_step(self.proposal_kind, D)
                if (tuple(ext_prop.shape) != (n_steps, Cn, T, raw) or ext_u is None
                        or tuple(ext_u.shape) != (n_steps, Cn, T)):
                    raise ValueError("ext_prop/ext_u shapes do not match [n_steps, n_chains, n_temps, raw]")
            a.trace = _opt(trace, "trace", self.state_dtype)
            a.trace_logp = _opt(trace_logp, "trace_logp", torch.float32)
            a.trace_every, a.trace_chains, a.trace_temps = 0, 0, 0
            if trace is not None:
                te = max(1, int(trace_every))
                rows = periodic_steps_in(step0, step0 + n_steps, te)
                if trace.dim() != 4 or trace.shape[3] != D or trace.shape[0] < trace_row0 + rows:
                    raise ValueError("trace must be [rows >= trace_row0 + traced steps, trace_chains, trace_temps, dim]")
                a.trace_every = te
                a.trace_chains = trace.shape[1]
                a.trace_temps = trace.shape[2]
            a.trace_row0 = trace_row0
            if accept_flags is not None and tuple(accept_flags.shape) != (n_steps, Cn, T):
                raise ValueError("accept_flags must be [n_steps, n_chains, n_temps]")
            a.accept_flags = _opt(accept_flags, "accept_flags", torch.uint8)
            self._plain = plain
            if trace is not None and ext_prop is None and ext_u is None and ext_swap_u is None and accept_flags is None:
                self._last_trace = (trace, trace_logp, trace_every)
        # ptrwm_run, or the accumulator's entry point with its struct in front of the stream; with anything else bound, the
        # first of ptrwm_run_with_diagnostics / _histogram / _adaptation / _ladder / _autocorr / _covariance / _energy that takes all that is bound: each
        # takes what the one before it takes and one struct more, behind the two accumulators (pooled, per chain)
        name, opt = ("ptrwm_run", ()) if self._mom is None else (self._MOMENT_KINDS[self._mom[0]][2], (self._mom[2],))
        blocks = (self._flow, self._hist, self._adapt, self._ladder, self._acf, self._cov, self._energy)
        if any(b is not None for b in blocks):
            more = [b[1] if b is not None else None for b in blocks]
            last = max(i for i, b in enumerate(more) if b is not None)
            name = self._RUN_WITH[last]
            kind, mom = (self._mom[0], self._mom[2]) if self._mom is not None else (None, None)
            opt = (mom if kind == "pooled" else None, mom if kind == "chain" else None, *more[:last + 1])
        with self._guard:
            rc = getattr(self._lib, name)(self._refs[2], self._refs[3], self._refs[4], *opt, _stream(self.device))
        if rc != 0:
            raise PTRWMError(rc, name)

    def _split_buffers(self):
        if getattr(self, "_split", None) is None:
            Cn, T, D = self.shape
            # proposals, and the two planes of the accept scratch (uniforms; the proposal's own squared jump or -1)
            self._split = (torch.empty(Cn, T, D, device=self.device, dtype=torch.float32),
                           torch.empty(2, Cn, T, device=self.device, dtype=torch.float32))
        return self._split

    def set_device_step(self, counter: Optional[torch.Tensor]) -> None:
        """Device-step mode of the split-step calls (include/ptrwm.h `device_step`): ``counter`` is a one-element int64
        device tensor; split_propose / split_accept then perform step ``counter + step`` - their ``step`` argument is an
        offset baked into the call - so the argument lists of a block of steps do not depend on where the run stands and
        the block can be captured in a HIP graph (``split_advance(n)`` adds n to the counter as its last node).  ``None``
        switches it off."""
        if counter is not None:
            if counter.numel() != 1 or counter.device != self.device:
                raise ValueError("device_step must be a one-element int64 tensor on the run's device")
            self._a.device_step = _require_device(counter, "device_step", torch.int64)
        else:
            self._a.device_step = None
        self._device_step = counter  # (kept alive)

    def split_advance(self, n: int = 1) -> None:
        """*device_step += n on the current stream (ptrwm_split_advance)."""
        if n < 1:
            raise ValueError("split_advance: n >= 1")
        self._a.n_steps = n
        with self._guard:
            rc = self._lib.ptrwm_split_advance(self._refs[4], _stream(self.device))
        if rc != 0:
            raise PTRWMError(rc, "ptrwm_split_advance")

    def split_propose(self, step: int, ext_prop: Optional[torch.Tensor] = None,
                      ext_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """First half of a split step (ptrwm_split_propose): returns the proposals [C, T, D] of global step ``step``
        (a buffer owned by the plan, overwritten by the next call).  The caller evaluates its log-density on them and
        passes the result to ``split_accept``."""
        a = self._a
        Cn, T, D = self.shape
        if self.state_dtype != torch.float32:
            raise TypeError("split steps take float32 states (float64 states: the fused kernel only)")
        props, acc_u = self._split_buffers()
        a.step0 = step
        self._last_trace = (None, None, None)
        a.ext_prop = _opt(ext_prop, "ext_prop", torch.float32)
        a.ext_u = _opt(ext_u, "ext_u", torch.float32)
        if ext_prop is not None:
            raw = ext_raw_per_step(self.proposal_kind, D)
            if tuple(ext_prop.shape) != (Cn, T, raw) or ext_u is None or tuple(ext_u.shape) != (Cn, T):
                raise ValueError("ext_prop / ext_u of one step must be [n_chains, n_temps, raw] / [n_chains, n_temps]")
        self._plain = False
        precond = self._precond
        if precond is not None:  # increments s_t L z (ptrwm_split_propose_precond)
            with self._guard:
                rc = self._lib.ptrwm_split_propose_precond(self._refs[3], self._refs[4], D, precond[1], props.data_ptr(),
                                                           acc_u.data_ptr(), _stream(self.device))
            if rc != 0:
                raise PTRWMError(rc, "ptrwm_split_propose_precond")
            return props
        with self._guard:
            rc = self._lib.ptrwm_split_propose(self._refs[3], self._refs[4], D, props.data_ptr(), acc_u.data_ptr(),
                                               _stream(self.device))
        if rc != 0:
            raise PTRWMError(rc, "ptrwm_split_propose")
        return props

    def set_preconditioner(self, chol: Optional[torch.Tensor]) -> None:
        """Bind the factor of a preconditioned Normal proposal (include/ptrwm.h ptrwm_precond_args): ``chol`` is a float32
        [dim, dim] tensor on the run's device, read on its lower triangle only; every following ``split_propose`` then
        proposes x + s_t L z through ptrwm_split_propose_precond.  The tensor's memory is what is bound: rewriting it in place
        (``precond_update``) changes the factor of the steps that follow, captured ones included.  ``None`` switches it off."""
        if chol is None:
            self._precond = None
            return
        D = self.shape[2]
        if self.proposal_kind != PROPOSAL_NORMAL:
            raise ValueError("a preconditioner needs the Normal proposal")
        self._precond = self._bind_block("preconditioner", PrecondArgs, {}, self._tuning_tensors(
            "preconditioner", (("chol", chol, torch.float32, (D, D), True),)))

    def set_precond_update(self, sxx: Optional[torch.Tensor], sx: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                           run_xx: Optional[torch.Tensor] = None, run_x: Optional[torch.Tensor] = None,
                           run_w: Optional[torch.Tensor] = None, *, windows: int = 1, probe_every: int = 1, memory: float = 0.5,
                           jitter: float = 1e-6,
                           min_count: Optional[float] = None, chol_history: Optional[torch.Tensor] = None,
                           weight_history: Optional[torch.Tensor] = None, skipped: Optional[torch.Tensor] = None) -> None:
        """What ``precond_update`` learns the bound factor from (include/ptrwm.h ptrwm_precond_update_args): the window sums
        ``sxx`` [dim, dim], ``sx`` [dim] float64 and ``count`` [1] int64 - ptrwm_covariance's of one temperature - and the
        running triple ``run_xx`` [dim, dim], ``run_x`` [dim], ``run_w`` [1] float64; ``chol_history`` [windows + 1, dim, dim]
        float32, ``weight_history`` [windows] float64 and ``skipped`` [1] int64 are optional records.  ``probe_every`` is the
        period of ``precond_probe``.  ``None`` switches it off."""
        if sxx is None:
            self._precond_update = self._precond_probe = None
            return
        if int(probe_every) < 1:
            raise ValueError("preconditioner probe_every must be >= 1")
        if self._precond is None:
            raise RuntimeError("set_precond_update: no preconditioner bound (set_preconditioner)")
        D, K = self.shape[2], int(windows)
        if K < 1:
            raise ValueError("preconditioner windows must be >= 1")
        f64, i64 = torch.float64, torch.int64
        pointers = self._tuning_tensors("preconditioner", (
            ("sxx", sxx, f64, (D, D), True), ("sx", sx, f64, (D,), True), ("count", count, i64, (1,), True),
            ("run_xx", run_xx, f64, (D, D), True), ("run_x", run_x, f64, (D,), True), ("run_w", run_w, f64, (1,), True),
            ("chol_history", chol_history, torch.float32, (K + 1, D, D), False),
            ("weight_history", weight_history, f64, (K,), False), ("skipped", skipped, i64, (1,), False)))
        self._precond_update = self._bind_block("preconditioner", PrecondUpdateArgs, dict(
            chol=self._precond[0].chol, memory=float(memory), jitter=float(jitter),
            min_count=float(4 * D if min_count is None else min_count), windows=K), pointers)
        # the probe: ptrwm_covariance of temperature 0 into the window's sums (their layout with temps = 1; the update's block
        # has checked them and keeps them alive)
        up = self._precond_update[0]
        self._precond_probe = self._bind_block("preconditioner", CovArgs, dict(
            temps=1, every=int(probe_every), sxx=up.sxx, sx=up.sx, count=up.count), ())

    def precond_probe(self, step: int) -> None:
        """One probe of the factor's tuning behind step ``step`` (ptrwm_covariance on temperature 0 into the bound window sums,
        driven with burn-in 0 and ``every`` = the probe period: a step whose step counter is no multiple of it adds nothing).
        Host-step mode: the call sits between blocks of steps, never inside a captured one."""
        if self._precond_probe is None:
            raise RuntimeError("precond_probe: no update bound (set_precond_update)")
        a = self._a
        burn_in, dstep = a.burn_in, a.device_step
        a.burn_in, a.device_step = 0, None
        try:
            self._split_call("ptrwm_covariance", self._precond_probe[1], step)
        finally:
            a.burn_in, a.device_step = burn_in, dstep

    def precond_update(self, window: int) -> None:
        """The factor's update of window ``window`` from the bound sums (ptrwm_precond_update): the bound ``chol`` is rewritten
        in place - or kept, and ``skipped`` counted, where the sums do not give a positive-definite matrix - and the window
        sums are left zero.  Enqueues one small kernel."""
        self._tuning_call("precond_update", self._precond_update, "update bound (set_precond_update)", window, extent=2)

    def split_accept(self, step: int, logp_proposed: torch.Tensor, ext_swap_u: Optional[torch.Tensor] = None,
                     accept_flags: Optional[torch.Tensor] = None, swap_event_offset: int = 0, no_sweep: bool = False) -> None:
        """Second half (ptrwm_split_accept): Metropolis rule on ``logp_proposed`` [C, T], updates, and the swap event
        when ``step`` is a swap step.  ``no_sweep`` (device-step mode only, PTRWM_SPLIT_NO_SWEEP): the caller's assertion
        that this step is not a swap step - the swap kernel is then not enqueued at all."""
        a = self._a
        Cn, T, D = self.shape
        props, acc_u = self._split_buffers()
        if tuple(logp_proposed.shape) != (Cn, T):
            raise ValueError(f"logp_proposed must be [{Cn}, {T}]")
        if ext_swap_u is not None and tuple(ext_swap_u.shape) != (Cn, T - 1):
            raise ValueError(f"ext_swap_u of one event must be [{Cn}, {T - 1}]")
        if accept_flags is not None and tuple(accept_flags.shape) != (Cn, T):
            raise ValueError(f"accept_flags of one step must be [{Cn}, {T}]")
        a.step0 = step
        a.swap_event_offset = swap_event_offset
        a.split_flags = 1 if no_sweep else 0
        self._last_trace = (None, None, None)
        a.ext_swap_u = _opt(ext_swap_u, "ext_swap_u", torch.float32)
        a.accept_flags = _opt(accept_flags, "accept_flags", torch.uint8)
        self._plain = False
        lp = _require_device(logp_proposed, "logp_proposed", torch.float32)
        try:
            if self._flow is not None:  # the flow update happens inside the swap kernel this enqueues
                with self._guard:
                    rc = self._lib.ptrwm_split_accept_with_flow(self._refs[4], D, props.data_ptr(), acc_u.data_ptr(), lp, self._flow[1], _stream(self.device))
            else:
                with self._guard:
                    rc = self._lib.ptrwm_split_accept(self._refs[4], D, props.data_ptr(), acc_u.data_ptr(), lp, _stream(self.device))
        finally:
            a.split_flags = 0  # (every other entry point requires 0)
        if rc != 0:
            raise PTRWMError(rc, "ptrwm_split_accept_with_flow" if self._flow is not None else "ptrwm_split_accept")

    def swap_sweep(self, rng_step: int, event_index: int, rng_stream: int = 2,
                   ext_swap_u: Optional[torch.Tensor] = None) -> None:
        """One stand-alone swap event over the current states (the reference's ``_attempt_all_swaps()`` called on
        its own).  Swap uniforms: ``ext_swap_u`` [C, T-1], else Philox stream ``rng_stream`` at step ``rng_step``
        (stream 1 = the stream the fused kernel's own swap events use)."""
        a = self._a
        Cn, T, D = self.shape
        if ext_swap_u is not None and tuple(ext_swap_u.shape) != (Cn, T - 1):
            raise ValueError(f"ext_swap_u must be [{Cn}, {T - 1}]")
        if a.device_step:
            raise RuntimeError("device-step mode is for split steps only: set_device_step(None) before swap_sweep()")
        a.step0 = rng_step
        self._last_trace = (None, None, None)
        a.ext_swap_u = _opt(ext_swap_u, "ext_swap_u", torch.float32)
        self._plain = False  # per-launch fields of _a were touched: the next launch() rewrites them
        if self._flow is not None:
            with self._guard:
                rc = self._lib.ptrwm_swap_sweep_with_flow(self._refs[4], D, event_index, rng_stream, self._flow[1], _stream(self.device))
        else:
            with self._guard:
                rc = self._lib.ptrwm_swap_sweep(self._refs[4], D, event_index, rng_stream, _stream(self.device))
        if rc != 0:
            raise PTRWMError(rc, "ptrwm_swap_sweep_with_flow" if self._flow is not None else "ptrwm_swap_sweep")


def run(
    target: Target,
    proposal: Proposal,
    *,
    state: torch.Tensor,  # [C, T, D] float32 (or float64: states, trace and ext_prop in double, include/ptrwm.h state_f64)
    logp: torch.Tensor,  # [C, T] float32
    beta: torch.Tensor,  # [T] float32
    step0: int,
    n_steps: int,
    burn_in: int = 0,
    swap_every: int = 1,
    swap_mode: int = SWAP_EXCHANGE,
    swap_order: int = ORDER_SEQUENTIAL,
    seed: int = 0,
    chain_offset: int = 0,
    n_accept: Optional[torch.Tensor] = None,  # [C, T] int64
    sq_jump: Optional[torch.Tensor] = None,  # [C, T] float64
    swap_accept: Optional[torch.Tensor] = None,  # [C, T] int64
    last_swap_ordinal: Optional[torch.Tensor] = None,  # [C, T] int64
    **per_launch,
) -> None:
    """One-shot form: enqueue ``n_steps`` fused MH(+swap) steps for every (chain, temperature) replica.
    ``per_launch``: ext_prop, ext_u, ext_swap_u, trace, trace_logp, trace_row0, trace_every, accept_flags."""
    RunPlan(target, proposal, state=state, logp=logp, beta=beta, burn_in=burn_in, swap_every=swap_every,
            swap_mode=swap_mode, swap_order=swap_order, seed=seed, chain_offset=chain_offset, n_accept=n_accept,
            sq_jump=sq_jump, swap_accept=swap_accept, last_swap_ordinal=last_swap_ordinal).launch(
        step0, n_steps, **per_launch)
