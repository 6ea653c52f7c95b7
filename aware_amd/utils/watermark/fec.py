"""Coded payloads (EXTENSION, no counterpart in the reference): a zero-terminated convolutional code of constraint length 7
with an optional CRC, and its soft-decision Viterbi decoder.  DESIGN.md section 29.  These numpy functions are the model the
device kernel (csrc/viterbi_kernels.hip, aware_viterbi_decode) is tested against, bit for bit.

The code.  `rate` "1/2" has the generators (0o171, 0o133), n = 2; "1/3" has (0o133, 0o171, 0o165), n = 3.  The encoder's
state s is 6 bits and starts at 0; for an input bit b, r = (b << 6) | s, output bit g is the parity of r & poly_g, and the
next state is r >> 1.

The frame of a detector with L outputs and a CRC of c in {0, 8, 16} bits: T = L // n trellis steps carry k = T - 6 - c
message bits, then the CRC of the message (MSB first), then 6 zeros; the n T coded bits fill the positions 0 .. n T - 1 and
the remaining L - n T positions are 0 and ignored by the decoder.  The CRC is bitwise, MSB first, not reflected, without a
final xor, its register initialised to all ones (so that the all-zero frame is not valid): CRC-8 has the polynomial 0x07,
CRC-16 0x1021.
"""
from __future__ import annotations

import numpy as np

RATES = {"1/2": (0o171, 0o133), "1/3": (0o133, 0o171, 0o165)}
CRC_POLY = {0: 0, 8: 0x07, 16: 0x1021}
TAIL = 6                                # zero bits that return the encoder to state 0
STATES = 64
MAX_BITS = 512                          # L of aware_viterbi_decode
MAX_ROWS = 1 << 20                      # R of aware_viterbi_decode
CODE_KEYS = ("rate", "crc")


def check_rate(rate) -> str:
    if rate not in RATES:
        raise ValueError(f"payload_code: rate = {rate!r}: one of {tuple(RATES)} is expected")
    return rate


def check_crc(crc) -> int:
    if isinstance(crc, bool) or not isinstance(crc, (int, np.integer)) or int(crc) not in CRC_POLY:
        raise ValueError(f"payload_code: crc = {crc!r}: one of {tuple(CRC_POLY)} is expected")
    return int(crc)


def check_payload_code(code):
    """The card key `payload_code`: None for no code, or a mapping with `rate` (required) and `crc` (default 0) ->
    {"rate", "crc"}.  ValueError for anything else, naming the key."""
    if code is None:
        return None
    if not isinstance(code, dict):
        raise ValueError(f"payload_code = {code!r}: a mapping with the keys {CODE_KEYS} is expected")
    unknown = sorted(set(code) - set(CODE_KEYS), key=str)
    if unknown:
        raise ValueError(f"payload_code: unknown key {unknown[0]!r}: the keys are {CODE_KEYS}")
    if "rate" not in code:
        raise ValueError("payload_code: the key 'rate' is missing")
    return {"rate": check_rate(code["rate"]), "crc": check_crc(code.get("crc", 0))}


def capacity(L: int, rate: str, crc: int) -> int:
    """The message bits k = L // n - 6 - crc of a frame over L detector outputs.  ValueError where k < 1."""
    n, c = len(RATES[check_rate(rate)]), check_crc(crc)
    k = int(L) // n - TAIL - c
    if k < 1:
        raise ValueError(f"payload_code: {int(L)} detector outputs at rate {rate} with a CRC of {c} bits leave {k} message "
                         f"bits; at least 1 is needed")
    return k


def crc_register(bits, crc: int) -> np.ndarray:
    """The CRC register after the bits [..., m] (0 / 1), per row: int64 [...]."""
    c = check_crc(crc)
    bits = np.asarray(bits).astype(np.int64)
    reg = np.full(bits.shape[:-1], (1 << c) - 1, dtype=np.int64)
    if c == 0:
        return reg
    poly, mask = CRC_POLY[c], (1 << c) - 1
    for i in range(bits.shape[-1]):
        fb = ((reg >> (c - 1)) ^ bits[..., i]) & 1
        reg = ((reg << 1) & mask) ^ (fb * poly)
    return reg


def crc_bits(bits, crc: int) -> np.ndarray:
    """The CRC of the bits [..., m] as crc bits, MSB first: int32 [..., crc]."""
    c = check_crc(crc)
    reg = crc_register(bits, c)
    return np.stack([(reg >> (c - 1 - j)) & 1 for j in range(c)], axis=-1).astype(np.int32) if c else \
        np.zeros(reg.shape + (0,), dtype=np.int32)


def conv_encode(inputs, rate: str) -> np.ndarray:
    """The coded bits of the input bits [..., T] from state 0: int32 [..., n T], step t at n t .. n t + n - 1."""
    polys = RATES[check_rate(rate)]
    inputs = np.asarray(inputs).astype(np.int64)
    out = np.zeros(inputs.shape[:-1] + (inputs.shape[-1] * len(polys),), dtype=np.int32)
    s = np.zeros(inputs.shape[:-1], dtype=np.int64)
    for t in range(inputs.shape[-1]):
        r = (inputs[..., t] << 6) | s
        for g, poly in enumerate(polys):
            out[..., len(polys) * t + g] = _parity(r & poly)
        s = r >> 1
    return out


def _parity(v) -> np.ndarray:
    v = np.asarray(v).astype(np.int64)
    p = np.zeros_like(v)
    for i in range(7):
        p ^= (v >> i) & 1
    return p


def message_bits(message, k: int) -> np.ndarray:
    """A message as k bits (int32): a bit array of exactly k bits, or bytes with 8 len <= k, MSB first, padded with zero
    bits at the end.  ValueError otherwise."""
    if isinstance(message, (bytes, bytearray)):
        bits = np.unpackbits(np.frombuffer(bytes(message), dtype=np.uint8)).astype(np.int32)
        if len(bits) > k:
            raise ValueError(f"message of {len(message)} bytes ({len(bits)} bits); the frame carries {k} bits")
        return np.concatenate([bits, np.zeros(k - len(bits), dtype=np.int32)])
    bits = np.asarray(message)
    if bits.ndim != 1 or len(bits) != k:
        raise ValueError(f"message of shape {bits.shape}; a bit array of exactly {k} bits (or bytes of at most {k // 8}) is expected")
    if not np.all((bits == 0) | (bits == 1)):
        raise ValueError("message: bits have to be 0 or 1")
    return bits.astype(np.int32)


def message_bytes(bits) -> bytes:
    """The first k // 8 bytes of k message bits, MSB first."""
    bits = np.asarray(bits).astype(np.uint8)
    return np.packbits(bits[:len(bits) // 8 * 8]).tobytes()


def encode_frame(message, L: int, rate: str, crc: int) -> np.ndarray:
    """The frame of a message for a detector of L outputs: int32 [L] of 0 / 1 (bipolar as bits2bipolar makes it)."""
    k = capacity(L, rate, crc)
    msg = message_bits(message, k)
    inputs = np.concatenate([msg, crc_bits(msg, crc), np.zeros(TAIL, dtype=np.int32)])
    coded = conv_encode(inputs, rate)
    return np.concatenate([coded, np.zeros(int(L) - len(coded), dtype=np.int32)])


def _branches(rate: str):
    """pred [64, 2]: the predecessor s_x of state d; sign [64, 2, n]: True where the branch's output bit is 1 (+1)."""
    polys = RATES[rate]
    d = np.arange(STATES)
    pred = np.stack([((d & 31) << 1) | x for x in (0, 1)], axis=1)
    r = ((d >> 5) << 6)[:, None] | pred
    sign = np.stack([_parity(r & poly) for poly in polys], axis=2).astype(bool)
    return pred, sign


def soft_values(values, centre: float) -> np.ndarray:
    """y = values - centre in float32, 0 where that is not finite (an erasure)."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.asarray(values, dtype=np.float32) - np.float32(centre)
    return np.where(np.isfinite(y), y, np.float32(0)).astype(np.float32)


def viterbi_decode(values, centre: float, rate: str, crc: int) -> dict:
    """values [R, L] float32 -> {"bits" int32 [R, T]: the decoded input bits (message, CRC, tail); "metric" float32 [R];
    "valid" bool [R]; "corrected" int32 [R]}.

    All arithmetic in float32.  y_i = v_i - centre, 0 where not finite.  Path metrics start at 0 for state 0 and -inf
    elsewhere.  At step t state d has the input bit d >> 5 and the predecessors s_x = ((d & 31) << 1) | x;
    m_x = ((pm[s_x] + sigma_0 y_nt) + sigma_1 y_nt+1) + sigma_2 y_nt+2, every addition rounded on its own, the signs applied
    by negation; x = 1 exactly where m_1 > m_0; pm'[d] = m_x.  Traceback from state 0 after step T - 1; metric = pm[0] then.
    valid: metric finite and (crc > 0) the decoded CRC equals the CRC of the decoded message.  corrected: the positions
    i < n T where (y_i > 0) differs from the re-encoded decoded sequence."""
    polys = RATES[check_rate(rate)]
    n, c = len(polys), check_crc(crc)
    v = np.asarray(values, dtype=np.float32)
    if v.ndim != 2:
        raise ValueError(f"viterbi_decode: values [R, L] are expected; got {v.shape}")
    R, L = v.shape
    k = capacity(L, rate, c)
    T = L // n
    y = soft_values(v, centre)
    pred, sign = _branches(rate)
    pm = np.full((R, STATES), -np.inf, dtype=np.float32)
    pm[:, 0] = 0
    surv = np.zeros((T, R, STATES), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            m = [pm[:, pred[:, x]] for x in (0, 1)]                    # [R, 64] each
            for g in range(n):
                yg = y[:, n * t + g][:, None]
                for x in (0, 1):
                    m[x] = (m[x] + np.where(sign[None, :, x, g], yg, -yg)).astype(np.float32)
            take = m[1] > m[0]
            surv[t] = take
            pm = np.where(take, m[1], m[0]).astype(np.float32)
    metric = pm[:, 0].copy()
    bits = np.zeros((R, T), dtype=np.int32)
    s = np.zeros(R, dtype=np.int64)
    rows = np.arange(R)
    for t in range(T - 1, -1, -1):
        bits[:, t] = s >> 5
        s = ((s & 31) << 1) | surv[t, rows, s]
    valid = np.isfinite(metric)
    if c:
        got = np.zeros(R, dtype=np.int64)
        for j in range(c):
            got = (got << 1) | bits[:, k + j]
        valid &= got == crc_register(bits[:, :k], c)
    corrected = np.count_nonzero((y[:, :n * T] > 0) != conv_encode(bits, rate).astype(bool), axis=1).astype(np.int32)
    return {"bits": bits, "metric": metric, "valid": valid, "corrected": corrected}


def pack_bits(bits) -> np.ndarray:
    """bits [R, T] -> uint32 [R, ceil(T / 32)], bit t at bit t % 32 of word t // 32: aware_viterbi_decode's words."""
    bits = np.asarray(bits).astype(np.uint64)
    R, T = bits.shape
    words = (T + 31) // 32
    padded = np.zeros((R, words * 32), dtype=np.uint64)
    padded[:, :T] = bits
    return (padded.reshape(R, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_bits(words, T: int) -> np.ndarray:
    """The inverse of pack_bits: uint32 [R, ceil(T / 32)] -> int32 [R, T]."""
    w = np.asarray(words).astype(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], -1)[:, :T].astype(np.int32)
