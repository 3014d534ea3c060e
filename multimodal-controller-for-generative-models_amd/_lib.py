"""ctypes binding of libmcgen_hip.so, derived from the C ABI in include/mcgen_hip.h (read by _abi.py): the header is the
only place a struct, a signature or a constant is written down."""
from __future__ import annotations

import ctypes as C
import os

from ._abi import Header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libmcgen_hip.so')

with open(os.path.join(os.path.dirname(_HERE), 'include', 'mcgen_hip.h')) as _f:
    HEADER = Header(_f.read())          # once per process, at import

Seg = HEADER.structs['mcgen_seg_t']
Conv = HEADER.structs['mcgen_conv_t']
ConvPlan = HEADER.structs['mcgen_conv_plan_t']
Wgrad = HEADER.structs['mcgen_wgrad_t']
WReduce = HEADER.structs['mcgen_wreduce_t']
PrepEx = HEADER.structs['mcgen_prepex_t']
Prep = HEADER.structs['mcgen_prep_t']
BnFin = HEADER.structs['mcgen_bn_fin_t']
Gated = HEADER.structs['mcgen_gated_t']
PxSample = HEADER.structs['mcgen_px_sample_t']
CGate = HEADER.structs['mcgen_cgate_t']
Code = HEADER.structs['mcgen_code_t']
AnAffine = HEADER.structs['mcgen_an_affine_t']
Pld = HEADER.structs['mcgen_pld_t']
Icw = HEADER.structs['mcgen_icw_t']
Icb = HEADER.structs['mcgen_icb_t']
Icp = HEADER.structs['mcgen_icp_t']
Icpb = HEADER.structs['mcgen_icpb_t']
AnBwd = HEADER.structs['mcgen_an_bwd_t']
Pcs = HEADER.structs['mcgen_pcs_t']
BnRun = HEADER.structs['mcgen_bn_run_t']
SnLayer = HEADER.structs['mcgen_sn_layer_t']
LecamState = HEADER.structs['mcgen_lecam_state_t']

CONSTANTS = HEADER.constants            # every #define and enumerator: MCGEN_ROUTE_*, MCGEN_*_MAX, ...
F32, BF16 = CONSTANTS['MCGEN_F32'], CONSTANTS['MCGEN_BF16']
WGRAD_MULTI_MAX = CONSTANTS['MCGEN_WGRAD_MULTI_MAX']

# every symbol include/mcgen_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {name: HEADER.symbol(name) for name in HEADER.functions}

_lib = None


class McgenError(RuntimeError):
    pass


def load():
    """Load the HIP library; raises (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise McgenError(f'{LIB_PATH} is missing: run __graft_entry__.build() '
                             f'(or csrc/build.sh); there is no CPU fallback')
        # PyTorch-ROCm ships its own libamdhip64; the process must have ONE HIP runtime, and it has to be the one torch's
        # streams and allocations live in: import torch first, so that this library's libamdhip64 dependency resolves to
        # the copy already loaded (loaded the other way round, every launch fails with "no ROCm-capable device").
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc: int, what: str = ''):
    if rc != 0:
        raise McgenError(f'{what}: {load().mcgen_last_error().decode()}')
