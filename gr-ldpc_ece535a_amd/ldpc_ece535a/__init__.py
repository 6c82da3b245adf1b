"""ldpc_ece535a -- MI355X-native drop-in for gr-ldpc_ece535a's decode path.

Python face of the package, mirroring the reference's SWIG module
(swig/ldpc_ece535a_swig.i:17-22, python/__init__.py:45):

    ldpc_ece535a.ldpc_decoder_cb(method)   # GR-3.7-shaped decoder block
    ldpc_ece535a.ldpc_encoder_bc()         # GR-3.7-shaped encoder block

plus the C-ABI binding (`Decoder`, `encode`, `reorder_h`, ...) of
include/ldpc_hip.h.  Decoding always runs on the GPU through
lib/libldpc_hip.so; there is no CPU fallback.
"""
from ._capi import (  # noqa: F401
    FLAG_NO_REORDER, FLAG_QC_TABLES, METHOD_BITFLIP, METHOD_HARD, METHOD_LOGDOMAIN, METHOD_SUMPRODUCT,
    PREC_F32, PREC_F64, PREC_F64_FAST, PREC_F64_LIBM, Decoder, LdpcError, bpsk_awgn, check_frame, count_bit_errors,
    default_h, encode, encode_qc, plan_layers, plan_layers_q8, plan_layout, plan_qc, plan_qc_encoder, plan_qc_q8,
    plan_rate_match, random_bits, rate_match, rate_recover, reorder_h,
    CRC6, CRC11, CRC16, CRC24A, CRC24B, CRC24C, CRCS, crc_attach, crc_bits, plan_crc,
)
from .blocks import (  # noqa: F401,E402
    STATE_IN_SYNC, STATE_IN_SYNC_INVERTED, STATE_OUT_OF_SYNC, ldpc_decoder_cb, ldpc_encoder_bc,
)
from . import flowgraph  # noqa: F401,E402
from .codes import qc_dual_diagonal, qc_encode, qc_expand, qc_parity_core  # noqa: F401,E402
