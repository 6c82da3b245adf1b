"""The code-block CRC contract (include/ldpc_hip.h), restated in numpy.

A CRC is (len, poly), poly the generator g without its leading term.  The
register starts at 0 and takes bits MSB first, with no reflection and no final
xor; over bits b_0 .. b_{n-1} it ends as (b_0 x^(n-1) + ... + b_{n-1}) x^len mod
g.  The block is the first A = K - filler information bits (column M + p for
position p): the payload, then the payload's register MSB first.  A block's
remainder is the block as a polynomial (position p has degree A - 1 - p) mod g:
the XOR of weights(len, poly, A)[p] over its one bits, which equals
register(payload) ^ the CRC field; 0 means pass.

`decode_crc` is what tests hold the layered decodes to while a CRC is set.  It
is built on the restatements tests/layered_ref.py and tests/layered_q8_ref.py
as they are: frames are independent and a stop does not change a trajectory, so
a restatement called with max_iters = k and a check period it never reaches
gives every frame's state at check point k."""
import numpy as np

CRC24A, CRC24B, CRC24C = (24, 0x864CFB), (24, 0x800063), (24, 0xB2B117)
CRC16, CRC11, CRC6 = (16, 0x1021), (11, 0x621), (6, 0x21)
NAMED = dict(CRC24A=CRC24A, CRC24B=CRC24B, CRC24C=CRC24C, CRC16=CRC16, CRC11=CRC11, CRC6=CRC6)
# the register over the 72 bits of ASCII "123456789", MSB first
KNOWN = dict(CRC16=0x31C3, CRC24A=0xCDE703, CRC24B=0x23EF52, CRC24C=0xF48279, CRC11=0x5CA,
             CRC6=0x15)
NEVER = 1 << 30   # a check period no decode reaches


def register(len, poly, bits):
    """The shift register, one bit at a time."""
    top, mask, r = 1 << (len - 1), (1 << len) - 1, 0
    for b in np.asarray(bits).reshape(-1):
        r ^= top if int(b) & 1 else 0
        r = ((r << 1) & mask) ^ (poly if r & top else 0)
    return r


def weights(len, poly, A):
    """w[p] = x^(A-1-p) mod g."""
    top, mask = 1 << (len - 1), (1 << len) - 1
    w, v = np.zeros(A, np.uint32), 1
    for p in range(A - 1, -1, -1):
        w[p] = v
        v = ((v << 1) & mask) ^ (poly if v & top else 0)
    return w


def remainder(len, poly, blocks):
    """blocks (B, A) bits -> (B,) uint32."""
    blocks = np.atleast_2d(np.asarray(blocks, np.uint8))
    w = weights(len, poly, blocks.shape[1])
    return np.bitwise_xor.reduce(np.where(blocks & 1, w[None, :], np.uint32(0)), axis=1)


def attach(len, poly, payload, K=None):
    """payload (B, A - len) bits -> (B, K) information bits: payload, CRC MSB
    first, K - A zero fillers (K None: no fillers)."""
    payload = np.atleast_2d(np.asarray(payload, np.uint8)) & 1
    B, P = payload.shape
    out = np.zeros((B, P + len if K is None else K), np.uint8)
    out[:, :P] = payload
    for b in range(B):
        r = register(len, poly, payload[b])
        out[b, P:P + len] = [(r >> (len - 1 - j)) & 1 for j in range(len)]
    return out


def check_points(cap, et_period):
    """The iterations after which the loop evaluates the syndrome."""
    return sorted(set(range(et_period, cap, et_period)) | {cap})


def decode_crc(ref_decode, csr, plan, y, cap, crc, A, mode, et_period=1, **kw):
    """ref_decode: layered_ref.decode or layered_q8_ref.decode (kw: its
    arithmetic).  mode "report" or "stop".  Returns bits, packed, iters, synd,
    llr and crc: a frame stops at its first check point with a zero syndrome
    weight, in stop mode a zero remainder, or the cap."""
    M, N = csr[0], csr[1]
    y = np.ascontiguousarray(y, np.float32).reshape(-1, N)
    B = y.shape[0]
    out = dict(bits=np.zeros((B, N), np.uint8), iters=np.zeros(B, np.int32),
               synd=np.zeros(B, np.int32), llr=np.zeros((B, N), np.float32),
               crc=np.zeros(B, np.uint32))
    live = np.arange(B)
    for k in check_points(cap, et_period):
        r = ref_decode(csr, plan, y[live], k, et_period=NEVER, **kw)
        rem = remainder(*crc, r["bits"][:, M:M + A])
        stop = r["synd"] == 0
        if mode == "stop":
            stop |= rem == 0
        if k == cap:
            stop[:] = True
        idx = live[stop]
        out["bits"][idx] = r["bits"][stop]
        out["iters"][idx] = k
        out["synd"][idx] = r["synd"][stop]
        out["llr"][idx] = r["llr"][stop]
        out["crc"][idx] = rem[stop]
        live = live[~stop]
        if live.size == 0:
            break
    out["packed"] = np.packbits(out["bits"][:, M:], axis=1)
    return out
