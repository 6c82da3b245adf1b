"""ctypes binding of the C ABI in include/ldpc_hip.h (lib/libldpc_hip.so).

The shared library is built in-tree (gr-ldpc_ece535a_amd/lib/); importing this
module never falls back to anything else: if the library is missing, loading
fails with an error that says how to build it, and if no GPU is usable,
Decoder() raises.
"""
import ctypes
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(PKG_ROOT, "lib")
HIP_LIB = os.path.join(LIB_DIR, "libldpc_hip.so")

METHOD_LOGDOMAIN, METHOD_SUMPRODUCT, METHOD_BITFLIP, METHOD_HARD = 0, 1, 2, 3
PREC_F64, PREC_F32, PREC_F64_LIBM, PREC_F64_FAST = 0, 1, 2, 3
FLAG_NO_REORDER = 1
FLAG_GRAPH = 2
FLAG_PLAIN_LAYOUT = 4
FLAG_ONCHIP = 8
FLAG_QC_TABLES = 16
TEST_SERVE_UNCHECKED, TEST_SERVE_EPOCH, TEST_SERVE_EPOCH_NOW, TEST_STREAM_OVERLAP = 1, 2, 3, 4
SERVE_EPOCH_LIMIT = (1 << 23) - (1 << 16)
# ldpc_math_probe's functions (test seam)
(PROBE_TANH_HALF, PROBE_TANH_HALF_MASKED, PROBE_TANH_HALF_SMALL3, PROBE_CHECK_MSG,
 PROBE_CHECK_MSG_PACKED, PROBE_CHECK_MSG_PACKED_LEAN, PROBE_CHECK_MSG_OPEN3, PROBE_DIV1,
 PROBE_DIV2, PROBE_DIV3) = range(10)
PATH_SMALL, PATH_GRAPH, PATH_ONCHIP = 0, 1, 2
MODE_LATENCY, MODE_THROUGHPUT = 0, 1
ERRORS = {0: "LDPC_OK", -1: "LDPC_EINVAL", -2: "LDPC_EUNSUPPORTED", -3: "LDPC_EDEVICE",
          -4: "LDPC_ESINGULAR", -5: "LDPC_ENOMEM", -6: "LDPC_ETIMEOUT"}


_u8p = ctypes.POINTER(ctypes.c_uint8)
_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_i = ctypes.c_int
_i64 = ctypes.c_int64
_vp = ctypes.c_void_p

# name -> (restype, argtypes); the full set the header declares
SIGNATURES = {
    "ldpc_default_h": (_i, [_u8p]),
    "ldpc_reorder_h": (_i, [_u8p, _i, _i, _i32p]),
    "ldpc_check_frame": (_i, [_u8p, _i, _i, _u8p, _i]),
    "ldpc_encode": (_i, [_u8p, _i, _i, _u8p, _i, _u8p]),
    "ldpc_create": (_vp, [_u8p, _i, _i, _i, _i]),
    "ldpc_create_csr": (_vp, [_i, _i, _i32p, _i32p, _i, _i]),
    "ldpc_ctx_csr": (_i, [_vp, _i32p, _i32p]),
    "ldpc_ctx_path": (_i, [_vp]),
    "ldpc_ctx_pipeline": (_i, [_vp, _i32p, _i32p]),
    "ldpc_ctx_layout": (_i, [_vp, _i32p]),
    "ldpc_plan_layout": (_i, [_u8p, _i, _i, _i, _i32p, _i32p, _i32p]),
    "ldpc_plan_storage_order": (_i, [_i, _i, _i32p, _i32p, _i32p, _i32p, _i64p]),
    "ldpc_plan_onchip": (_i, [_i, _i, _i, _i, _i, _i, _i, _i64p, _i32p]),
    "ldpc_set_work_limit": (_i, [_vp, _i64]),
    "ldpc_encode_device": (_i, [_vp, _vp, _i, _vp, _vp]),
    "ldpc_random_bits": (_i, [_vp, _i64, ctypes.c_uint64, _vp]),
    "ldpc_bpsk_awgn": (_i, [_vp, _i64, ctypes.c_float, ctypes.c_uint64, _vp, _vp]),
    "ldpc_count_bit_errors": (_i, [_vp, _vp, _i64, _i, _vp, _vp]),
    "ldpc_destroy": (None, [_vp]),
    "ldpc_last_error": (ctypes.c_char_p, [_vp]),
    "ldpc_ctx_info": (_i, [_vp, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p]),
    "ldpc_ctx_h": (_i, [_vp, _u8p]),
    "ldpc_decode": (_i, [_vp, _i, _i, _i, _i, _f32p, _i, _u8p, _u8p, _i32p, _i32p]),
    "ldpc_decode_strided": (_i, [_vp, _i, _i, _i, _i, _f32p, _i64, _i64, _i, ctypes.c_float, _i,
                                 _u8p, _u8p, _i32p, _i32p, _f32p]),
    "ldpc_decode_device": (_i, [_vp, _i, _i, _i, _i, _vp, _i64, _i, ctypes.c_float, _i,
                                _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldpc_decode_strided_both": (_i, [_vp, _i, _i, _i, _i, _f32p, _i64, _i64, _i,
                                     ctypes.c_float, _i, _u8p, _i32p]),
    "ldpc_decode_windows": (_i, [_vp, _i, _i, _i, _i, _f32p, _i64, _i, _i,
                                 ctypes.POINTER(ctypes.c_int64), _i, _u8p, _i32p]),
    "ldpc_stage_span": (_i, [_vp, _f32p, _i64, _i, _i]),
    "ldpc_serve_begin": (_i, [_vp, _i, _i, _i, _i]),
    "ldpc_serve_windows": (_i, [_vp, ctypes.POINTER(ctypes.c_int64), _i, _u8p, _i32p]),
    "ldpc_serve_end": (_i, [_vp]),
    "ldpc_ctx_streams": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_void_p)]),
    "ldpc_alist_read": (_i, [ctypes.c_char_p, _i32p, _i32p, _i32p, _i32p, _i64]),
    "ldpc_set_waves_per_cu": (_i, [_vp, _i]),
    "ldpc_set_launch_mode": (_i, [_vp, _i]),
    "ldpc_set_schedule": (_i, [_vp, _i]),
    "ldpc_synchronize": (_i, [_vp]),
    "ldpc_test_hook": (_i, [_vp, _i, _i64]),
    "ldpc_math_probe": (_i, [_vp, _i, _i, _vp, _vp, _i64, _vp]),
    "ldpc_ring_begin": (_i, [_vp, _i, _i, _i, _i, _vp]),
    "ldpc_ring_post": (_i64, [_vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "ldpc_ring_wait": (_i, [_vp, _i64]),
    "ldpc_ring_end": (_i, [_vp]),
    "ldpc_ring_info": (_i, [_vp, _i32p, _i32p]),
    "ldpc_plan_layers": (_i, [_i, _i, _i32p, _i32p, _i, _i32p, _i32p, _i64p, _i32p]),
    "ldpc_plan_qc": (_i, [_i, _i, _i, _i32p, _i, _i32p, _i32p, _i64p, _i32p]),
    "ldpc_plan_qc_encoder": (_i, [_i, _i, _i, _i32p, _i32p, _i32p, _i64p]),
    "ldpc_encode_qc": (_i, [_i, _i, _i, _i32p, _u8p, _i, _u8p]),
    "ldpc_create_qc": (_vp, [_i, _i, _i, _i32p, _i, _i]),
    "ldpc_ctx_qc": (_i, [_vp, _i32p, _i32p, _i32p, _i32p]),
    "ldpc_ctx_layers": (_i, [_vp, _i32p]),
    "ldpc_set_layers": (_i, [_vp, _i32p]),
    "ldpc_decode_layered": (_i, [_vp, ctypes.c_double, _i, _i, _i, _f32p, _i64, _i64, _i,
                                 ctypes.c_float, _i, _u8p, _u8p, _i32p, _i32p, _f32p]),
    "ldpc_decode_layered_device": (_i, [_vp, ctypes.c_double, _i, _i, _i, _vp, _i64, _i,
                                        ctypes.c_float, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldpc_plan_layers_q8": (_i, [_i, _i, _i32p, _i32p, _i32p, _i32p, _i64p, _i32p]),
    "ldpc_plan_qc_q8": (_i, [_i, _i, _i, _i32p, _i64p, _i32p]),
    "ldpc_decode_layered_q8": (_i, [_vp, _i, ctypes.c_float, _i, _i, _f32p, _i64, _i64, _i,
                                    ctypes.c_float, _i, _u8p, _u8p, _i32p, _i32p, _f32p]),
    "ldpc_decode_layered_q8_device": (_i, [_vp, _i, ctypes.c_float, _i, _i, _vp, _i64, _i,
                                           ctypes.c_float, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldpc_plan_rate_match": (_i64, [_i, _i, _i, _i, _i, _i, _i32p, _i32p, _i32p, _i32p]),
    "ldpc_rate_match": (_i, [_i, _i, _i, _i, _i, _i, _i, _u8p, _i, _u8p, _i64]),
    "ldpc_rate_recover": (_i, [_i, _i, _i, _i, _i, _f32p, _i64, _i64, ctypes.c_float,
                               ctypes.c_float, _i, _i, _i32p, _i32p, _f32p]),
    "ldpc_set_rate_match": (_i, [_vp, _i, _i, _i]),
    "ldpc_rate_match_device": (_i, [_vp, _vp, _i, _i, _i, _vp, _i64, _vp]),
    "ldpc_rate_recover_device": (_i, [_vp, _vp, _i64, ctypes.c_float, ctypes.c_float, _i, _i,
                                      _i32p, _i32p, _vp, _vp]),
    "ldpc_decode_layered_rm": (_i, [_vp, ctypes.c_double, _i, _i, _i, _f32p, _i64, _i64,
                                    ctypes.c_float, _i, _i32p, _i32p, ctypes.c_float, _i, _u8p,
                                    _u8p, _i32p, _i32p, _f32p]),
    "ldpc_decode_layered_rm_device": (_i, [_vp, ctypes.c_double, _i, _i, _i, _vp, _i64,
                                           ctypes.c_float, _i, _i32p, _i32p, ctypes.c_float, _i,
                                           _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldpc_decode_layered_q8_rm": (_i, [_vp, _i, ctypes.c_float, _i, _i, _f32p, _i64, _i64,
                                       ctypes.c_float, _i, _i32p, _i32p, ctypes.c_float, _i, _u8p,
                                       _u8p, _i32p, _i32p, _f32p]),
    "ldpc_decode_layered_q8_rm_device": (_i, [_vp, _i, ctypes.c_float, _i, _i, _vp, _i64,
                                              ctypes.c_float, _i, _i32p, _i32p, ctypes.c_float, _i,
                                              _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldpc_crc_bits": (_i64, [_i, ctypes.c_uint32, _u8p, _i64]),
    "ldpc_plan_crc": (_i, [_i, _i, _i, _i, ctypes.c_uint32, _u32p]),
    "ldpc_crc_attach": (_i, [_i, _i, _i, _i, ctypes.c_uint32, _u8p, _i, _u8p]),
    "ldpc_set_crc": (_i, [_vp, _i, ctypes.c_uint32, _i]),
    "ldpc_crc_results": (_i, [_vp, _u32p, _i]),
    "ldpc_crc_results_device": (_vp, [_vp]),
    "ldpc_crc_attach_device": (_i, [_vp, _vp, _i, _vp, _vp]),
    "ldpc_crc_check_device": (_i, [_vp, _vp, _i, _vp, _vp]),
}

RM_MAX_TX = 4
UNRECEIVED_LCI = 2.0 ** -100   # what a column no sample reaches gets, by default

# the code-block CRCs by name: (len, poly), poly without the leading term
CRC24A, CRC24B, CRC24C = (24, 0x864CFB), (24, 0x800063), (24, 0xB2B117)
CRC16, CRC11, CRC6 = (16, 0x1021), (11, 0x621), (6, 0x21)
CRCS = {"CRC24A": CRC24A, "CRC24B": CRC24B, "CRC24C": CRC24C, "CRC16": CRC16, "CRC11": CRC11,
        "CRC6": CRC6}
CRC_REPORT, CRC_STOP = 0, 1

_lib = None


class LdpcError(RuntimeError):
    pass


def lib():
    """Load lib/libldpc_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(HIP_LIB):
            raise LdpcError("%s is missing: build it with `make -C %s` (or "
                            "__graft_entry__.build()); there is no fallback" % (HIP_LIB, PKG_ROOT))
        L = ctypes.CDLL(HIP_LIB)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _check(rc, ctx=None):
    if rc < 0:
        msg = lib().ldpc_last_error(ctx)
        raise LdpcError("%s: %s" % (ERRORS.get(rc, rc), (msg or b"").decode()))
    return rc


def default_h():
    """The reference decoder's 32x64 H (lib/ldpc_decoder_cb_impl.cc:63-96)."""
    H = np.zeros((32, 64), np.uint8)
    _check(lib().ldpc_default_h(_p(H, _u8p)))
    return H


def reorder_h(H):
    """reorderHMatrix (lib/ldpc_decoder_cb_impl.cc:255-307) -> (Hr, chosen)."""
    H = np.ascontiguousarray(H, np.uint8).copy()
    M, N = H.shape
    chosen = np.zeros(M, np.int32)
    _check(lib().ldpc_reorder_h(_p(H, _u8p), M, N, _p(chosen, _i32p)))
    return H, chosen


def check_frame(H, bits, threshold):
    """checkFrame (lib/ldpc_decoder_cb_impl.cc:236-253)."""
    H = np.ascontiguousarray(H, np.uint8)
    bits = np.ascontiguousarray(bits, np.uint8)
    M, N = H.shape
    return _check(lib().ldpc_check_frame(_p(H, _u8p), M, N, _p(bits, _u8p), int(threshold)))


def encode(Hr, data_bits):
    """makeParityCheck (lib/ldpc_encoder_bc_impl.cc:275-294): (B, N-M) data
    bits -> (B, N) codewords [parity; data]."""
    Hr = np.ascontiguousarray(Hr, np.uint8)
    M, N = Hr.shape
    d = np.ascontiguousarray(np.atleast_2d(data_bits), np.uint8)
    out = np.zeros((d.shape[0], N), np.uint8)
    _check(lib().ldpc_encode(_p(Hr, _u8p), M, N, _p(d, _u8p), d.shape[0], _p(out, _u8p)))
    return out


def plan_layout(H, reorder=True, plain=False):
    """The small-code kernel's LDS layout for H (host only, no GPU): dict with
    cell (E,) = lane slot of each edge in CSR order of the decoder's H, pos (N,)
    = lane position of each column, and model = {searched, cc, ec, plain_cc,
    plain_ec}: modelled extra LDS bank-conflict cycles per iteration of the
    column-centric sum-product / min-sum kernels for this layout and for the
    plain CSR layout (csrc/ldpc_layout.hpp)."""
    H = np.ascontiguousarray(H, np.uint8)
    M, N = H.shape
    flags = (0 if reorder else FLAG_NO_REORDER) | (FLAG_PLAIN_LAYOUT if plain else 0)
    cell = np.zeros(M * N, np.int32)
    pos = np.zeros(N, np.int32)
    model = np.zeros(5, np.int32)
    E = _check(lib().ldpc_plan_layout(_p(H, _u8p), M, N, flags, _p(cell, _i32p), _p(pos, _i32p),
                                      _p(model, _i32p)))
    return dict(cell=cell[:E].copy(), pos=pos,
                model=dict(zip(("searched", "cc", "ec", "plain_cc", "plain_ec"),
                               (int(v) for v in model))))


def plan_storage_order(csr):
    """The large-code min-sum pipeline's storage order for csr = (M, N,
    row_ptr, col_idx) (host only, no GPU): dict with order (0 identity, 1
    DVB-S2 residue classes), rpos (M,) and cpos (N,) = storage position of
    each original row / column, and score = contiguity of the identity and
    residue-class orders (-1: not tried)."""
    M, N, rp, ci = csr
    rp = np.ascontiguousarray(rp, np.int32)
    ci = np.ascontiguousarray(ci, np.int32)
    rpos = np.zeros(M, np.int32)
    cpos = np.zeros(N, np.int32)
    score = np.zeros(2, np.int64)
    order = _check(lib().ldpc_plan_storage_order(M, N, _p(rp, _i32p), _p(ci, _i32p),
                                                 _p(rpos, _i32p), _p(cpos, _i32p),
                                                 _p(score, _i64p)))
    return dict(order=order, rpos=rpos, cpos=cpos, score=(int(score[0]), int(score[1])))


def plan_onchip(M, N, E, dc_max, dv_max, method=METHOD_SUMPRODUCT, precision=PREC_F64):
    """ldpc_plan_onchip (host only, no GPU): dict with fits (the on-chip
    kernels take a code of this shape for this method and precision),
    lds_bytes (LDS its workgroup declares: the frame's state, plus the code's
    tables where they fit behind it) and threads (of the workgroup)."""
    lds, threads = ctypes.c_int64(0), ctypes.c_int32(0)
    fits = _check(lib().ldpc_plan_onchip(int(M), int(N), int(E), int(dc_max), int(dv_max),
                                         int(method), int(precision), ctypes.byref(lds),
                                         ctypes.byref(threads)))
    return dict(fits=bool(fits), lds_bytes=lds.value, threads=threads.value)


def plan_layers(csr, precision=PREC_F64):
    """ldpc_plan_layers (host only, no GPU) for csr = (M, N, row_ptr, col_idx):
    dict with fits (the layered kernel takes the code at this precision),
    layer_of_row (M,), n_layers, lds_bytes (LDS its workgroup declares: the
    frame's state, plus the code's tables where they fit behind it; the frame's
    state alone when the code does not fit) and threads (of the workgroup)."""
    M, N, rp, ci = csr
    rp = np.ascontiguousarray(rp, np.int32)
    ci = np.ascontiguousarray(ci, np.int32)
    plan = np.zeros(max(int(M), 1), np.int32)
    L, lds, threads = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
    fits = _check(lib().ldpc_plan_layers(int(M), int(N), _p(rp, _i32p), _p(ci, _i32p),
                                         int(precision), _p(plan, _i32p), ctypes.byref(L),
                                         ctypes.byref(lds), ctypes.byref(threads)))
    return dict(fits=bool(fits), layer_of_row=plan[:M], n_layers=L.value, lds_bytes=lds.value,
                threads=threads.value)


def _qc_base(base, Z):
    """A base matrix as a contiguous (mb, nb) int32 array, with Z as an int."""
    base = np.ascontiguousarray(base, np.int32)
    if base.ndim != 2:
        raise LdpcError("LDPC_EINVAL: a base matrix is two-dimensional (mb, nb)")
    return base, int(Z)


def plan_qc(base, Z, precision=PREC_F64):
    """ldpc_plan_qc (host only, no GPU) for the quasi-cyclic code of base
    matrix `base` ((mb, nb) shifts, -1 = no circulant) and lifting size Z: dict
    with fits (the circulant kernel takes the code at this precision),
    lds_bytes (LDS its workgroup declares: one frame's state), threads (of the
    workgroup, 64 * ceil(Z / 64)) and csr = (M, N, row_ptr, col_idx), the
    expanded H."""
    base, Z = _qc_base(base, Z)
    mb, nb = base.shape
    ok = mb >= 1 and nb >= 1 and 1 <= Z <= 1024 and ((base >= -1) & (base < Z)).all()
    M, N, E = (mb * Z, nb * Z, Z * int((base >= 0).sum())) if ok else (0, 0, 0)
    rp = np.zeros(M + 1, np.int32)
    ci = np.zeros(max(E, 1), np.int32)
    lds, threads = ctypes.c_int64(0), ctypes.c_int32(0)
    # a description the library refuses gets no buffers: it raises before it writes
    fits = _check(lib().ldpc_plan_qc(mb, nb, Z, _p(base, _i32p), int(precision),
                                     _p(rp, _i32p) if ok else None,
                                     _p(ci, _i32p) if ok else None, ctypes.byref(lds),
                                     ctypes.byref(threads)))
    return dict(fits=bool(fits), lds_bytes=lds.value, threads=threads.value,
                csr=(M, N, rp, ci[:E]))


def plan_layers_q8(csr):
    """ldpc_plan_layers_q8 (host only, no GPU): plan_layers for the fixed-point
    layered decoder's table route -- the same plan, lds_bytes = a16(2 N) +
    a16(E) + 128 plus the tables where they fit behind it."""
    M, N, rp, ci = csr
    rp = np.ascontiguousarray(rp, np.int32)
    ci = np.ascontiguousarray(ci, np.int32)
    plan = np.zeros(max(int(M), 1), np.int32)
    L, lds, threads = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
    fits = _check(lib().ldpc_plan_layers_q8(int(M), int(N), _p(rp, _i32p), _p(ci, _i32p),
                                            _p(plan, _i32p), ctypes.byref(L), ctypes.byref(lds),
                                            ctypes.byref(threads)))
    return dict(fits=bool(fits), layer_of_row=plan[:M], n_layers=L.value, lds_bytes=lds.value,
                threads=threads.value)


def plan_qc_q8(base, Z):
    """ldpc_plan_qc_q8 (host only, no GPU): plan_qc for the fixed-point layered
    decoder's circulant route, without the expansion: dict with fits, lds_bytes
    (one frame: a16(2 N) + a16(E) + 128) and threads."""
    base, Z = _qc_base(base, Z)
    lds, threads = ctypes.c_int64(0), ctypes.c_int32(0)
    fits = _check(lib().ldpc_plan_qc_q8(base.shape[0], base.shape[1], Z, _p(base, _i32p),
                                        ctypes.byref(lds), ctypes.byref(threads)))
    return dict(fits=bool(fits), lds_bytes=lds.value, threads=threads.value)


def plan_qc_encoder(base, Z):
    """ldpc_plan_qc_encoder (host only, no GPU): whether the quasi-cyclic code
    (base, Z) has a systematic encoder here (a dual-diagonal core, a block
    lower triangular extension, or both: include/ldpc_hip.h).  dict with
    encodable, core (the core's block rows, 0 for none), levels (of the step
    program: the device encoder's barriers), lds_bytes (of its workgroup) and,
    when not encodable, reason (naming the block row and column that broke the
    form).  Raises for a bad description."""
    base, Z = _qc_base(base, Z)
    core, levels, lds = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    ok = _check(lib().ldpc_plan_qc_encoder(base.shape[0], base.shape[1], Z, _p(base, _i32p),
                                           ctypes.byref(core), ctypes.byref(levels),
                                           ctypes.byref(lds)))
    out = dict(encodable=bool(ok), core=core.value, levels=levels.value, lds_bytes=lds.value)
    if not ok:
        out["reason"] = (lib().ldpc_last_error(None) or b"").decode()
    return out


def encode_qc(base, Z, data_bits):
    """ldpc_encode_qc (host only, no GPU): (B, K) data bits (bit 0 of each byte
    counts) -> (B, N) codewords [parity | data] of the quasi-cyclic code
    (base, Z), by the step program the device encoder runs."""
    base, Z = _qc_base(base, Z)
    mb, nb = base.shape
    d = np.ascontiguousarray(np.atleast_2d(data_bits), np.uint8)
    if d.shape[1] != (nb - mb) * Z:
        raise LdpcError("LDPC_EINVAL: data_bits must be (B, (nb - mb) * Z)")
    out = np.zeros((d.shape[0], nb * Z), np.uint8)
    _check(lib().ldpc_encode_qc(mb, nb, Z, _p(base, _i32p), _p(d, _u8p), d.shape[0],
                                _p(out, _u8p)))
    return out


_tx_memo = {}


def _tx_arrays(tx):
    """A call's transmissions [(k0, E), ...] as two C int32 arrays and the sum
    of E.  Kept per list: a decode call per batch would otherwise spend more
    time building them than the launch takes."""
    key = tuple((int(k0), int(e)) for k0, e in tx)
    hit = _tx_memo.get(key)
    if hit is None:
        if len(_tx_memo) >= 64:
            _tx_memo.clear()
        arr = ctypes.c_int32 * len(key)
        hit = _tx_memo[key] = (arr(*[k0 for k0, _ in key]), arr(*[e for _, e in key]),
                               sum(max(e, 0) for _, e in key))
    return hit


def plan_rate_match(M, N, punct, filler, ncb, tx):
    """ldpc_plan_rate_match (host only, no GPU): the pattern (punct, filler,
    ncb) on an M x N code and the transmissions tx = [(k0, E), ...] of one
    call.  dict with total (the samples per frame, sum E), col (total,) = the
    column of every sample, and count (N,) = the samples that reach each
    column, -1 for a filler.  Raises LDPC_EINVAL, the message naming the
    offending value, for what include/ldpc_hip.h refuses."""
    k0, e, n = _tx_arrays(tx)
    col = np.zeros(max(n, 1), np.int32)
    count = np.zeros(max(int(N), 1), np.int32)
    total = _check(lib().ldpc_plan_rate_match(int(M), int(N), int(punct), int(filler), int(ncb),
                                              len(k0), k0, e,
                                              _p(col, _i32p), _p(count, _i32p)))
    return dict(total=int(total), col=col[:total], count=count[:N])


def rate_match(M, N, punct, filler, ncb, k0, E, bits):
    """ldpc_rate_match (host only, no GPU): the bit selection of one
    transmission, (B, N) codeword bytes -> (B, E) bytes."""
    bits = np.ascontiguousarray(np.atleast_2d(bits), np.uint8)
    if bits.shape[1] != N:
        raise LdpcError("LDPC_EINVAL: bits must be (B, N)")
    out = np.zeros((bits.shape[0], max(int(E), 1)), np.uint8)
    _check(lib().ldpc_rate_match(int(M), int(N), int(punct), int(filler), int(ncb), int(k0),
                                 int(E), _p(bits, _u8p), bits.shape[0], _p(out, _u8p),
                                 out.shape[1]))
    return out[:, :int(E)]


def rate_recover(M, N, punct, filler, ncb, tx, rx, polarity=1.0, unreceived_lci=UNRECEIVED_LCI,
                 rx_stride=None, B=None):
    """ldpc_rate_recover (host only, no GPU): the soft combine of the received
    samples rx (frame b's transmissions concatenated at b * rx_stride) into
    (B, N) samples y = -Lci, which any decode takes at polarity 1."""
    k0, e, n = _tx_arrays(tx)
    x = np.ascontiguousarray(rx, np.float32).reshape(-1)
    if rx_stride is None:
        rx_stride = n
    if B is None:
        B = x.size // rx_stride if rx_stride else 0
    out = np.zeros((B, int(N)), np.float32)
    _check(lib().ldpc_rate_recover(int(M), int(N), int(punct), int(filler), int(ncb),
                                   _p(x, _f32p), x.size, int(rx_stride), float(polarity),
                                   float(unreceived_lci), int(B), len(k0), k0,
                                   e, _p(out, _f32p)))
    return out


def crc_bits(len, poly, bits):
    """ldpc_crc_bits (host only, no GPU): the CRC register (start 0, MSB
    first, no reflection, no final xor) over a 1-D array of bits."""
    b = np.ascontiguousarray(bits, np.uint8).reshape(-1)
    return int(_check(lib().ldpc_crc_bits(int(len), int(poly), _p(b, _u8p), b.size)))


def plan_crc(M, N, filler, len, poly):
    """ldpc_plan_crc (host only, no GPU): checks the CRC on an M x N code whose
    pattern has `filler` fillers.  Returns {A, weights}: the block is the first
    A = K - filler information bits, weights[p] = x^(A-1-p) mod g."""
    A = _check(lib().ldpc_plan_crc(int(M), int(N), int(filler), int(len), int(poly), None))
    w = np.zeros(A, np.uint32)
    _check(lib().ldpc_plan_crc(int(M), int(N), int(filler), int(len), int(poly), _p(w, _u32p)))
    return dict(A=A, weights=w)


def crc_attach(M, N, filler, len, poly, payload):
    """ldpc_crc_attach (host only, no GPU): payload (B, A - len) bits -> (B, K)
    information bits: the payload, its CRC MSB first, `filler` zeros."""
    A = _check(lib().ldpc_plan_crc(int(M), int(N), int(filler), int(len), int(poly), None))
    p = np.ascontiguousarray(payload, np.uint8)
    if p.ndim != 2 or p.shape[1] != A - int(len):
        raise LdpcError("LDPC_EINVAL: payload must be (B, A - len) = (B, %d)" % (A - int(len)))
    out = np.zeros((p.shape[0], int(N) - int(M)), np.uint8)
    _check(lib().ldpc_crc_attach(int(M), int(N), int(filler), int(len), int(poly), _p(p, _u8p),
                                 p.shape[0], _p(out, _u8p)))
    return out


class Decoder:
    """One decode context (device tables + stream) for one H.

    H: dense (M, N) 0/1 matrix (reorderHMatrix applied unless reorder=False),
    or csr=(M, N, row_ptr, col_idx) for a sparse H used as given.
    force_graph=True selects the large-code (HBM message) kernels even for a
    code the small-code kernel could take; plain_layout=True keeps the
    small-code kernel's edges and columns in CSR order (A/B and tests);
    onchip=True runs min-sum / sum-product on the on-chip kernels (one frame
    per workgroup, messages in LDS; path == PATH_ONCHIP) for any code that
    fits them (plan_onchip), and raises for one that does not.
    qc=(base, Z) builds the context of a quasi-cyclic code from its base matrix
    ((mb, nb) shifts, -1 = no circulant) and lifting size: the context
    Decoder(csr=plan_qc(base, Z)["csr"]) would be, except that its layered
    decodes take the block rows as their plan and, while that plan is in force,
    run the circulant kernel; qc_tables=True keeps the plan and runs the
    per-edge table kernel (A/B and tests)."""

    def __init__(self, H=None, reorder=True, device=0, csr=None, force_graph=False,
                 plain_layout=False, onchip=False, qc=None, qc_tables=False):
        flags = ((0 if reorder else FLAG_NO_REORDER) | (FLAG_GRAPH if force_graph else 0) |
                 (FLAG_PLAIN_LAYOUT if plain_layout else 0) | (FLAG_ONCHIP if onchip else 0) |
                 (FLAG_QC_TABLES if qc_tables else 0))
        if qc is not None:
            base, Z = _qc_base(*qc)
            self._ctx = lib().ldpc_create_qc(base.shape[0], base.shape[1], Z, _p(base, _i32p),
                                             flags, int(device))
            what = "ldpc_create_qc"
        elif csr is not None:
            M, N, rp, ci = csr
            rp = np.ascontiguousarray(rp, np.int32)
            ci = np.ascontiguousarray(ci, np.int32)
            self._ctx = lib().ldpc_create_csr(int(M), int(N), _p(rp, _i32p), _p(ci, _i32p),
                                              flags, int(device))
            what = "ldpc_create_csr"
        else:
            if H is None:
                H = default_h()
            H = np.ascontiguousarray(H, np.uint8)
            M, N = H.shape
            self._ctx = lib().ldpc_create(_p(H, _u8p), M, N, flags, int(device))
            what = "ldpc_create"
        if not self._ctx:
            raise LdpcError("%s failed: %s" % (what, lib().ldpc_last_error(None).decode()))
        v = [ctypes.c_int32(0) for _ in range(7)]
        _check(lib().ldpc_ctx_info(self._ctx, *[ctypes.byref(x) for x in v]), self._ctx)
        self.M, self.N, self.E, self.K, self.KB, self.dc_max, self.dv_max = [x.value for x in v]
        self.path = _check(lib().ldpc_ctx_path(self._ctx), self._ctx)
        self.row_ptr = np.zeros(self.M + 1, np.int32)
        self.col_idx = np.zeros(self.E, np.int32)
        _check(lib().ldpc_ctx_csr(self._ctx, _p(self.row_ptr, _i32p), _p(self.col_idx, _i32p)),
               self._ctx)
        self._H = None

    @property
    def qc(self):
        """ldpc_ctx_qc: (base, Z) of a quasi-cyclic context (base: the (mb, nb)
        shifts), None for any other."""
        v = [ctypes.c_int32(0) for _ in range(3)]
        if not _check(lib().ldpc_ctx_qc(self._ctx, *[ctypes.byref(x) for x in v], None), self._ctx):
            return None
        base = np.zeros((v[0].value, v[1].value), np.int32)
        _check(lib().ldpc_ctx_qc(self._ctx, None, None, None, _p(base, _i32p)), self._ctx)
        return base, v[2].value

    def pipeline(self):
        """ldpc_ctx_pipeline: {frames_per_chunk, chunks} of the large-code
        min-sum pipeline (both 0 when this context does not use it)."""
        f, c = ctypes.c_int32(0), ctypes.c_int32(0)
        _check(lib().ldpc_ctx_pipeline(self._ctx, ctypes.byref(f), ctypes.byref(c)), self._ctx)
        return {"frames_per_chunk": f.value, "chunks": c.value}

    @property
    def layout_model(self):
        """ldpc_ctx_layout: {searched, cc, ec, plain_cc, plain_ec} (see plan_layout)."""
        m = np.zeros(5, np.int32)
        _check(lib().ldpc_ctx_layout(self._ctx, _p(m, _i32p)), self._ctx)
        return dict(zip(("searched", "cc", "ec", "plain_cc", "plain_ec"), (int(v) for v in m)))

    @property
    def H(self):
        """The decoder's (reordered) H as a dense (M, N) array (built on demand)."""
        if self._H is None:
            self._H = np.zeros((self.M, self.N), np.uint8)
            _check(lib().ldpc_ctx_h(self._ctx, _p(self._H, _u8p)), self._ctx)
        return self._H

    def close(self):
        if getattr(self, "_ctx", None):
            lib().ldpc_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._ctx

    def decode(self, llr, method=METHOD_SUMPRODUCT, max_iters=50, et_period=1,
               precision=PREC_F64, polarity=1.0, cw_stride=None, elem_stride=1, B=None,
               want_bits=True, want_llr=False):
        """Decode host float32 frames (synchronous).  Returns a dict with
        packed (B,KB), bits (B,N), iters (B,), synd (B,) [, llr (B,N)]."""
        x = np.ascontiguousarray(llr, np.float32).reshape(-1)
        if cw_stride is None:
            cw_stride = self.N * elem_stride
        if B is None:
            B = x.size // cw_stride if cw_stride else 0
        packed = np.zeros((B, self.KB), np.uint8)
        bits = np.zeros((B, self.N), np.uint8) if want_bits else None
        iters = np.zeros(B, np.int32)
        synd = np.zeros(B, np.int32)
        post = np.zeros((B, self.N), np.float32) if want_llr else None
        _check(lib().ldpc_decode_strided(self._ctx, int(method), int(max_iters), int(et_period),
                                         int(precision), _p(x, _f32p), x.size, int(cw_stride),
                                         int(elem_stride), float(polarity), int(B),
                                         _p(packed, _u8p), _p(bits, _u8p), _p(iters, _i32p),
                                         _p(synd, _i32p), _p(post, _f32p)), self._ctx)
        out = dict(packed=packed, iters=iters, synd=synd)
        if want_bits:
            out["bits"] = bits
        if want_llr:
            out["llr"] = post
        return out

    def decode_both(self, llr, method=METHOD_SUMPRODUCT, max_iters=50, et_period=1,
                    precision=PREC_F64, polarity=1.0, cw_stride=None, elem_stride=1, B=None):
        """ldpc_decode_strided_both: the B windows decoded at +polarity (rows
        0..B-1) and -polarity (rows B..2B-1) in one launch.  Returns dict with
        packed (2B,KB) and synd (2B,)."""
        x = np.ascontiguousarray(llr, np.float32).reshape(-1)
        if cw_stride is None:
            cw_stride = self.N * elem_stride
        if B is None:
            B = x.size // cw_stride if cw_stride else 0
        packed = np.zeros((2 * B, self.KB), np.uint8)
        synd = np.zeros(2 * B, np.int32)
        _check(lib().ldpc_decode_strided_both(self._ctx, int(method), int(max_iters),
                                              int(et_period), int(precision), _p(x, _f32p),
                                              x.size, int(cw_stride), int(elem_stride),
                                              float(polarity), int(B), _p(packed, _u8p),
                                              _p(synd, _i32p)), self._ctx)
        return dict(packed=packed, synd=synd)

    def stage_span(self, samples, elem_stride=1, max_windows=0):
        """ldpc_stage_span: copy a sample span to the device for the
        decode_windows(..., reuse_span=True) calls that follow."""
        x = np.ascontiguousarray(samples, np.float32).reshape(-1)
        self._span = x  # the copy is asynchronous: keep the source alive
        _check(lib().ldpc_stage_span(self._ctx, _p(x, _f32p), x.size, int(elem_stride),
                                     int(max_windows)), self._ctx)

    def decode_windows(self, samples, windows, method=METHOD_SUMPRODUCT, max_iters=50,
                       et_period=1, precision=PREC_F64, elem_stride=1, reuse_span=False):
        """ldpc_decode_windows: windows (B,) int64 = (start << 1) | negate over
        one host sample span.  Returns dict(packed (B,KB), synd (B,))."""
        x = np.ascontiguousarray(samples, np.float32).reshape(-1)
        w = np.ascontiguousarray(windows, np.int64)
        B = w.size
        packed = np.zeros((B, self.KB), np.uint8)
        synd = np.zeros(B, np.int32)
        _check(lib().ldpc_decode_windows(self._ctx, int(method), int(max_iters), int(et_period),
                                         int(precision), _p(x, _f32p), x.size, int(elem_stride),
                                         1 if reuse_span else 0,
                                         w.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B,
                                         _p(packed, _u8p), _p(synd, _i32p)), self._ctx)
        return dict(packed=packed, synd=synd)

    def serve_begin(self, method=METHOD_SUMPRODUCT, max_iters=5, precision=PREC_F64,
                    max_windows=4096):
        """ldpc_serve_begin: start the window server over the span staged last
        (stage_span); rounds then go through serve_windows."""
        _check(lib().ldpc_serve_begin(self._ctx, int(method), int(max_iters), int(precision),
                                      int(max_windows)), self._ctx)

    def serve_windows(self, windows):
        """ldpc_serve_windows: one round of windows (int64 (start << 1) | negate)
        of the staged span.  Returns dict(packed (B,KB), synd (B,))."""
        w = np.ascontiguousarray(windows, np.int64)
        B = w.size
        packed = np.zeros((B, self.KB), np.uint8)
        synd = np.zeros(B, np.int32)
        _check(lib().ldpc_serve_windows(self._ctx, w.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                        B, _p(packed, _u8p), _p(synd, _i32p)), self._ctx)
        return dict(packed=packed, synd=synd)

    def streams(self, n):
        """ldpc_ctx_streams: n hipStream_t handles (ints) of the context's
        in-flight set (best effort: self.streams_distinct of them distinct)."""
        arr = (ctypes.c_void_p * int(n))()
        self.streams_distinct = _check(lib().ldpc_ctx_streams(self._ctx, int(n), arr), self._ctx)
        return [int(x) for x in arr]

    def ring_begin(self, method=METHOD_SUMPRODUCT, max_iters=50, et_period=1,
                   precision=PREC_F64, stream=None):
        """ldpc_ring_begin: open a frame-ring session (one persistent launch for
        every batch posted until ring_end), after the work on `stream`."""
        _check(lib().ldpc_ring_begin(self._ctx, int(method), int(max_iters), int(et_period),
                                     int(precision), stream), self._ctx)

    def ring_post(self, d_in, B, d_packed, d_iters=None, d_synd=None, cw_stride=None):
        """ldpc_ring_post: post B device-resident frames (raw pointers); returns
        the batch id."""
        if cw_stride is None:
            cw_stride = self.N
        ptr = lambda x: None if x is None else int(x)  # noqa: E731
        return _check(lib().ldpc_ring_post(self._ctx, ptr(d_in), int(cw_stride), int(B),
                                           ptr(d_packed), ptr(d_iters), ptr(d_synd)), self._ctx)

    def ring_wait(self, batch):
        """ldpc_ring_wait: return once batch `batch` is complete."""
        _check(lib().ldpc_ring_wait(self._ctx, int(batch)), self._ctx)

    def ring_end(self):
        """ldpc_ring_end: end the session (work enqueued on the session's
        stream afterwards follows its last batch)."""
        _check(lib().ldpc_ring_end(self._ctx), self._ctx)

    def ring_info(self):
        """ldpc_ring_info: {launches, workgroups} of this context's ring."""
        a, b = ctypes.c_int32(0), ctypes.c_int32(0)
        _check(lib().ldpc_ring_info(self._ctx, ctypes.byref(a), ctypes.byref(b)), self._ctx)
        return {"launches": a.value, "workgroups": b.value}

    def test_hook(self, op, arg=0):
        """ldpc_test_hook (test seam): TEST_SERVE_UNCHECKED, TEST_SERVE_EPOCH,
        TEST_SERVE_EPOCH_NOW."""
        return _check(lib().ldpc_test_hook(self._ctx, int(op), int(arg)), self._ctx)

    def math_probe(self, fn, precision, d_a, n, d_out, d_b=None):
        """ldpc_math_probe (test seam): function `fn` (PROBE_*) of the kernels'
        arithmetic at `precision` on n device reals at d_a (and d_b), to d_out;
        enqueued on the context's stream."""
        return _check(lib().ldpc_math_probe(self._ctx, int(fn), int(precision), d_a, d_b, int(n),
                                            d_out), self._ctx)

    def serve_end(self):
        _check(lib().ldpc_serve_end(self._ctx), self._ctx)

    def decode_device(self, d_in, B, d_packed, method=METHOD_SUMPRODUCT, max_iters=50,
                      et_period=1, precision=PREC_F64, polarity=1.0, cw_stride=None,
                      elem_stride=1, d_bits=None, d_iters=None, d_synd=None, d_llr=None,
                      stream=None):
        """Enqueue a decode of device-resident buffers (raw pointers / ints)."""
        if cw_stride is None:
            cw_stride = self.N * elem_stride
        _check(lib().ldpc_decode_device(self._ctx, int(method), int(max_iters), int(et_period),
                                        int(precision), d_in, int(cw_stride), int(elem_stride),
                                        float(polarity), int(B), d_packed, d_bits, d_iters,
                                        d_synd, d_llr, stream), self._ctx)

    @property
    def layers(self):
        """ldpc_ctx_layers: the layer of every row (M,) in the layered
        decoder's plan in force (the planner's -- on a quasi-cyclic context
        the block rows -- until set_layers replaces it)."""
        plan = np.zeros(self.M, np.int32)
        _check(lib().ldpc_ctx_layers(self._ctx, _p(plan, _i32p)), self._ctx)
        return plan

    def set_layers(self, layer_of_row):
        """ldpc_set_layers: a caller's plan (M layer indices; no two rows of a
        layer may share a column), or None for the planner's.  A refused plan
        raises and leaves the current one in force."""
        if layer_of_row is not None:
            layer_of_row = np.ascontiguousarray(layer_of_row, np.int32)
            if layer_of_row.shape != (self.M,):
                raise LdpcError("LDPC_EINVAL: a plan has one layer index per row (%d)" % self.M)
        _check(lib().ldpc_set_layers(self._ctx, _p(layer_of_row, _i32p)), self._ctx)

    def decode_layered(self, llr, scale=1.0, max_iters=50, et_period=1, precision=PREC_F64,
                       polarity=1.0, cw_stride=None, elem_stride=1, B=None, want_bits=True,
                       want_llr=False):
        """ldpc_decode_layered: layered normalized min-sum of host float32
        frames (synchronous); arguments and result as decode()."""
        x = np.ascontiguousarray(llr, np.float32).reshape(-1)
        if cw_stride is None:
            cw_stride = self.N * elem_stride
        if B is None:
            B = x.size // cw_stride if cw_stride else 0
        packed = np.zeros((B, self.KB), np.uint8)
        bits = np.zeros((B, self.N), np.uint8) if want_bits else None
        iters = np.zeros(B, np.int32)
        synd = np.zeros(B, np.int32)
        post = np.zeros((B, self.N), np.float32) if want_llr else None
        _check(lib().ldpc_decode_layered(self._ctx, float(scale), int(max_iters), int(et_period),
                                         int(precision), _p(x, _f32p), x.size, int(cw_stride),
                                         int(elem_stride), float(polarity), int(B),
                                         _p(packed, _u8p), _p(bits, _u8p), _p(iters, _i32p),
                                         _p(synd, _i32p), _p(post, _f32p)), self._ctx)
        out = self._with_crc(dict(packed=packed, iters=iters, synd=synd), B)
        if want_bits:
            out["bits"] = bits
        if want_llr:
            out["llr"] = post
        return out

    def decode_layered_device(self, d_in, B, d_packed, scale=1.0, max_iters=50, et_period=1,
                              precision=PREC_F64, polarity=1.0, cw_stride=None, elem_stride=1,
                              d_bits=None, d_iters=None, d_synd=None, d_llr=None, stream=None):
        """ldpc_decode_layered_device: enqueue a layered decode of
        device-resident buffers (raw pointers / ints), as decode_device()."""
        if cw_stride is None:
            cw_stride = self.N * elem_stride
        _check(lib().ldpc_decode_layered_device(self._ctx, float(scale), int(max_iters),
                                                int(et_period), int(precision), d_in,
                                                int(cw_stride), int(elem_stride), float(polarity),
                                                int(B), d_packed, d_bits, d_iters, d_synd, d_llr,
                                                stream), self._ctx)

    def decode_layered_q8(self, llr, num=16, llr_scale=8.0, max_iters=50, et_period=1,
                          polarity=1.0, cw_stride=None, elem_stride=1, B=None, want_bits=True,
                          want_llr=False):
        """ldpc_decode_layered_q8: fixed-point layered normalized min-sum
        (int8 messages, factor num / 16, samples scaled by llr_scale and
        rounded into [-127, 127]) of host float32 frames (synchronous);
        arguments and result as decode_layered()."""
        x = np.ascontiguousarray(llr, np.float32).reshape(-1)
        if cw_stride is None:
            cw_stride = self.N * elem_stride
        if B is None:
            B = x.size // cw_stride if cw_stride else 0
        packed = np.zeros((B, self.KB), np.uint8)
        bits = np.zeros((B, self.N), np.uint8) if want_bits else None
        iters = np.zeros(B, np.int32)
        synd = np.zeros(B, np.int32)
        post = np.zeros((B, self.N), np.float32) if want_llr else None
        _check(lib().ldpc_decode_layered_q8(self._ctx, int(num), float(llr_scale), int(max_iters),
                                            int(et_period), _p(x, _f32p), x.size, int(cw_stride),
                                            int(elem_stride), float(polarity), int(B),
                                            _p(packed, _u8p), _p(bits, _u8p), _p(iters, _i32p),
                                            _p(synd, _i32p), _p(post, _f32p)), self._ctx)
        out = self._with_crc(dict(packed=packed, iters=iters, synd=synd), B)
        if want_bits:
            out["bits"] = bits
        if want_llr:
            out["llr"] = post
        return out

    def decode_layered_q8_device(self, d_in, B, d_packed, num=16, llr_scale=8.0, max_iters=50,
                                 et_period=1, polarity=1.0, cw_stride=None, elem_stride=1,
                                 d_bits=None, d_iters=None, d_synd=None, d_llr=None, stream=None):
        """ldpc_decode_layered_q8_device: enqueue a fixed-point layered decode
        of device-resident buffers, as decode_layered_device()."""
        if cw_stride is None:
            cw_stride = self.N * elem_stride
        _check(lib().ldpc_decode_layered_q8_device(self._ctx, int(num), float(llr_scale),
                                                   int(max_iters), int(et_period), d_in,
                                                   int(cw_stride), int(elem_stride),
                                                   float(polarity), int(B), d_packed, d_bits,
                                                   d_iters, d_synd, d_llr, stream), self._ctx)

    def set_crc(self, len=0, poly=0, mode="report"):
        """ldpc_set_crc: the code-block CRC (len, poly) -- e.g. *CRC16 -- that
        every layered decode of this context checks: the block is the first
        A = K - filler information bits, payload then CRC.  mode "report": the
        decode is the plain decode and the remainders are one more output;
        "stop": a zero remainder also ends a frame, wherever the syndrome is
        evaluated.  The host decodes then return them as "crc" (0 = pass);
        crc_results() reads those of a device decode.  len = 0 or mode None
        turns the CRC off (the default)."""
        if mode is None or int(len) == 0:
            len, poly, m = 0, 0, CRC_REPORT
        elif mode in ("report", "stop"):
            m = CRC_STOP if mode == "stop" else CRC_REPORT
        else:
            raise LdpcError("LDPC_EINVAL: mode must be 'report', 'stop' or None (got %r)" % (mode,))
        _check(lib().ldpc_set_crc(self._ctx, int(len), int(poly), m), self._ctx)
        self._crc = (int(len), int(poly)) if int(len) else None

    def crc_results(self, n):
        """ldpc_crc_results: the remainders of the first n frames of the last
        layered decode (uint32, 0 = pass), once that decode has finished."""
        out = np.zeros(int(n), np.uint32)
        _check(lib().ldpc_crc_results(self._ctx, _p(out, _u32p), int(n)), self._ctx)
        return out

    def crc_results_device(self):
        """ldpc_crc_results_device: the device address of the remainders of the
        last layered decode (None before one), valid until the next decode."""
        return lib().ldpc_crc_results_device(self._ctx)

    def _with_crc(self, out, B):
        if getattr(self, "_crc", None):
            out["crc"] = self.crc_results(B)
        return out

    def crc_attach_device(self, d_payload, B, d_info, stream=None):
        """ldpc_crc_attach_device: (B, A - len) payload bytes on the device ->
        (B, K) information bits (payload, CRC, zero fillers), what
        encode_device takes."""
        _check(lib().ldpc_crc_attach_device(self._ctx, d_payload, int(B), d_info, stream),
               self._ctx)

    def crc_check_device(self, d_packed, B, d_rem, stream=None):
        """ldpc_crc_check_device: the remainders (uint32, 0 = pass) of (B, KB)
        packed information bits on the device, as any decode stores them."""
        _check(lib().ldpc_crc_check_device(self._ctx, d_packed, int(B), d_rem, stream), self._ctx)

    def set_rate_match(self, punct=0, filler=0, ncb=0):
        """ldpc_set_rate_match: the context's rate-matching pattern
        (include/ldpc_hip.h): transmit positions [0, punct) are never sent, the
        last `filler` information bits are known zeros and never sent, and the
        circular buffer is positions [punct, punct + ncb) (ncb = 0: to the
        end).  (0, 0, 0), the default, is the identity.  A refused pattern
        raises and leaves the current one in force."""
        _check(lib().ldpc_set_rate_match(self._ctx, int(punct), int(filler), int(ncb)), self._ctx)

    def rate_match_device(self, d_codewords, B, k0, E, d_out, out_stride=None, stream=None):
        """ldpc_rate_match_device: the E bytes transmission (k0, E) sends of
        each of B device codewords (B, N), frame b's at d_out + b * out_stride
        (default E)."""
        _check(lib().ldpc_rate_match_device(self._ctx, d_codewords, int(B), int(k0), int(E), d_out,
                                            int(E if out_stride is None else out_stride), stream),
               self._ctx)

    def rate_recover_device(self, d_rx, B, tx, d_samples, polarity=1.0,
                            unreceived_lci=UNRECEIVED_LCI, rx_stride=None, stream=None):
        """ldpc_rate_recover_device: the soft combine of B frames of received
        samples (the transmissions tx = [(k0, E), ...] concatenated, frame b at
        d_rx + b * rx_stride floats, default sum E) into (B, N) device samples
        y = -Lci, which any decode of this context takes at polarity 1."""
        k0, e, n = _tx_arrays(tx)
        _check(lib().ldpc_rate_recover_device(self._ctx, d_rx,
                                              int(n if rx_stride is None else rx_stride),
                                              float(polarity), float(unreceived_lci), int(B),
                                              len(k0), k0, e, d_samples,
                                              stream), self._ctx)

    def _rm_host(self, fn, head, rx, tx, max_iters, et_period, polarity, unreceived_lci,
                 rx_stride, B, want_bits, want_llr):
        k0, e, n = _tx_arrays(tx)
        x = np.ascontiguousarray(rx, np.float32).reshape(-1)
        if rx_stride is None:
            rx_stride = n
        if B is None:
            B = x.size // rx_stride if rx_stride else 0
        packed = np.zeros((B, self.KB), np.uint8)
        bits = np.zeros((B, self.N), np.uint8) if want_bits else None
        iters = np.zeros(B, np.int32)
        synd = np.zeros(B, np.int32)
        post = np.zeros((B, self.N), np.float32) if want_llr else None
        _check(fn(self._ctx, *head, _p(x, _f32p), x.size, int(rx_stride), float(polarity),
                  len(k0), k0, e, float(unreceived_lci), int(B),
                  _p(packed, _u8p), _p(bits, _u8p), _p(iters, _i32p), _p(synd, _i32p),
                  _p(post, _f32p)), self._ctx)
        out = self._with_crc(dict(packed=packed, iters=iters, synd=synd), B)
        if want_bits:
            out["bits"] = bits
        if want_llr:
            out["llr"] = post
        return out

    def decode_layered_rm(self, rx, tx, scale=1.0, max_iters=50, et_period=1, precision=PREC_F64,
                          polarity=1.0, unreceived_lci=UNRECEIVED_LCI, rx_stride=None, B=None,
                          want_bits=True, want_llr=False):
        """ldpc_decode_layered_rm: decode_layered of rate-matched host samples:
        frame b is the transmissions tx = [(k0, E), ...] of the context's
        pattern (set_rate_match) concatenated at b * rx_stride floats (default
        sum E), recovered by the kernel's frame load.  unreceived_lci is the
        Lci of a column no sample reaches: the default 2**-100 breaks the
        float contract's sign(0) = 0 tie, with which (0.0 is legal) a punctured
        column silences its rows."""
        head = (float(scale), int(max_iters), int(et_period), int(precision))
        return self._rm_host(lib().ldpc_decode_layered_rm, head, rx, tx, max_iters, et_period,
                             polarity, unreceived_lci, rx_stride, B, want_bits, want_llr)

    def decode_layered_q8_rm(self, rx, tx, num=16, llr_scale=8.0, max_iters=50, et_period=1,
                             polarity=1.0, unreceived_lci=UNRECEIVED_LCI, rx_stride=None, B=None,
                             want_bits=True, want_llr=False):
        """ldpc_decode_layered_q8_rm: decode_layered_q8 of rate-matched host
        samples, as decode_layered_rm (a filler quantises to +127, an
        unreceived column to 0)."""
        head = (int(num), float(llr_scale), int(max_iters), int(et_period))
        return self._rm_host(lib().ldpc_decode_layered_q8_rm, head, rx, tx, max_iters, et_period,
                             polarity, unreceived_lci, rx_stride, B, want_bits, want_llr)

    def decode_layered_rm_device(self, d_rx, B, tx, d_packed, scale=1.0, max_iters=50,
                                 et_period=1, precision=PREC_F64, polarity=1.0,
                                 unreceived_lci=UNRECEIVED_LCI, rx_stride=None, d_bits=None,
                                 d_iters=None, d_synd=None, d_llr=None, stream=None):
        """ldpc_decode_layered_rm_device: enqueue decode_layered_rm on
        device-resident buffers (raw pointers / ints)."""
        k0, e, n = _tx_arrays(tx)
        _check(lib().ldpc_decode_layered_rm_device(
            self._ctx, float(scale), int(max_iters), int(et_period), int(precision), d_rx,
            int(n if rx_stride is None else rx_stride), float(polarity), len(k0), k0,
            e, float(unreceived_lci), int(B), d_packed, d_bits, d_iters, d_synd, d_llr,
            stream), self._ctx)

    def decode_layered_q8_rm_device(self, d_rx, B, tx, d_packed, num=16, llr_scale=8.0,
                                    max_iters=50, et_period=1, polarity=1.0,
                                    unreceived_lci=UNRECEIVED_LCI, rx_stride=None, d_bits=None,
                                    d_iters=None, d_synd=None, d_llr=None, stream=None):
        """ldpc_decode_layered_q8_rm_device: enqueue decode_layered_q8_rm on
        device-resident buffers."""
        k0, e, n = _tx_arrays(tx)
        _check(lib().ldpc_decode_layered_q8_rm_device(
            self._ctx, int(num), float(llr_scale), int(max_iters), int(et_period), d_rx,
            int(n if rx_stride is None else rx_stride), float(polarity), len(k0), k0,
            e, float(unreceived_lci), int(B), d_packed, d_bits, d_iters, d_synd, d_llr,
            stream), self._ctx)

    def set_launch_mode(self, mode):
        """MODE_LATENCY (default: one decode at a time) or MODE_THROUGHPUT
        (several decodes in flight on different streams)."""
        _check(lib().ldpc_set_launch_mode(self._ctx, int(mode)), self._ctx)

    def set_waves_per_cu(self, n):
        _check(lib().ldpc_set_waves_per_cu(self._ctx, int(n)), self._ctx)

    def encode_device(self, d_data, B, d_codewords, stream=None):
        """Enqueue a systematic encode of B frames (device pointers): (B, K)
        0/1 bytes -> (B, N) codewords [parity | data]."""
        _check(lib().ldpc_encode_device(self._ctx, d_data, int(B), d_codewords, stream),
               self._ctx)

    def set_work_limit(self, nbytes):
        """Large-code path: device workspace cap (0 = default 8 GiB)."""
        _check(lib().ldpc_set_work_limit(self._ctx, int(nbytes)), self._ctx)

    def set_schedule(self, mode):
        """0 auto, 1 one wave per frame, 2 one workgroup per frame."""
        _check(lib().ldpc_set_schedule(self._ctx, int(mode)), self._ctx)

    def synchronize(self):
        _check(lib().ldpc_synchronize(self._ctx), self._ctx)


def alist_read(path):
    """ldpc_alist_read: a MacKay alist file as (M, N, row_ptr, col_idx)."""
    M, N = ctypes.c_int32(0), ctypes.c_int32(0)
    bpath = os.fsencode(path)
    E = lib().ldpc_alist_read(bpath, ctypes.byref(M), ctypes.byref(N), None, None, 0)
    if E < 0:
        raise LdpcError("ldpc_alist_read(%s): %s" % (path, lib().ldpc_last_error(None).decode()))
    rp = np.zeros(M.value + 1, np.int32)
    ci = np.zeros(max(E, 1), np.int32)
    _check(lib().ldpc_alist_read(bpath, ctypes.byref(M), ctypes.byref(N), _p(rp, _i32p),
                                 _p(ci, _i32p), int(E)))
    return M.value, N.value, rp, ci[:E]


def random_bits(d_out, n, seed, stream=None):
    """n seeded random 0/1 bytes into device memory (Philox4x32-10)."""
    _check(lib().ldpc_random_bits(d_out, int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, stream))


def bpsk_awgn(d_bits, n, sigma, seed, d_out, stream=None):
    """d_out = 2 * bits - 1 + sigma * N(0, 1) (float32, device pointers)."""
    _check(lib().ldpc_bpsk_awgn(d_bits, int(n), float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                d_out, stream))


def count_bit_errors(d_a, d_b, per_frame, B, d_counts, stream=None):
    """Per-frame count of differing 0/1 bytes (device pointers)."""
    _check(lib().ldpc_count_bit_errors(d_a, d_b, int(per_frame), int(B), d_counts, stream))
