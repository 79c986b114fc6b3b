"""References for lfamd_flash_attn_q (include/lfamd_hip.h): flash attention on a Q8_0 / Q4_0 K and V cache.

The inputs are fattn_ref's with K and V passed through `quantise` — tests/cpy_ref.quantize on the f32 values, the bytes lfamd_cpy would
store — and the call gets those raw blocks.  The operands as a route sees them:
    n_q <= 8   f32 d * code (exact in f32)
    n_q > 8    f16(d * code), rounded once to nearest even
and the reference is fattn_ref.ref64 on them, the emulation fattn_ref.emulate on them: from the operands on, the routes are
lfamd_flash_attn's, so the tolerances are fattn_ref's TOL_F32 and TOL_MMA, unchanged.

Shapes as in fattn_ref; raw K / V are uint8 [ne3][n_head_kv][n_kv][D / 32 * block size]."""
import numpy as np

import cpy_ref
import fattn_ref as R
from llamafile_amd import ggml_types as T

TYPES = (T.Q8_0, T.Q4_0)
BLOCK = {T.Q8_0: 34, T.Q4_0: 18}


def row_bytes(t, D):
    return D // 32 * BLOCK[t]


def quantise(t, X):
    """f32 (or f16) values [..., D] -> raw blocks uint8 [..., D / 32 * block size]."""
    X = np.asarray(X, np.float32)
    raw = cpy_ref.quantize(t, X)
    return np.ascontiguousarray(raw.reshape(X.shape[:-1] + (row_bytes(t, X.shape[-1]),)))


def codes_and_d(t, raw):
    """(d f32 [..., blocks, 1], codes f32 [..., blocks, 32]) of raw blocks."""
    b = raw.reshape(raw.shape[:-1] + (-1, BLOCK[t]))
    d = np.ascontiguousarray(b[..., :2]).view(np.float16).astype(np.float32)
    pay = b[..., 2:]
    if t == T.Q8_0:
        codes = pay.view(np.int8).astype(np.float32)
    else:  # element j < 16: the low nibble of byte j; element j + 16: its high nibble
        codes = np.concatenate([pay & 15, pay >> 4], axis=-1).astype(np.float32) - np.float32(8)
    return d, codes


def dequantise(t, raw):
    """The f32 d * code, [..., D]."""
    d, codes = codes_and_d(t, raw)
    return (d * codes).astype(np.float32).reshape(raw.shape[:-1] + (-1,))


def as_route_sees(route, X32):
    """The dequantised values as the route's arithmetic takes them: f32, or f16 rounded once (n_q > 8)."""
    return X32 if route == "decode" else X32.astype(np.float16)


def inputs_of(case, t, seed=0):
    """(Q, raw K, raw V, K, V, mask, scale): K / V are the operands as the case's route sees them."""
    Q, K, V, mask, scale = R.inputs_of(case, seed=seed)
    route = R.route_of(case[4])
    Kraw, Vraw = quantise(t, K), quantise(t, V)
    return Q, Kraw, Vraw, as_route_sees(route, dequantise(t, Kraw)), as_route_sees(route, dequantise(t, Vraw)), mask, scale


# ---- the device suite's cases (tests/test_gpu_flash_attn_q.py), also what tests/test_fattn_q_ref.py measures the emulation on
def decode_edge_cases():
    """fattn_ref.decode_edge_cases() without the 512- and 513-chunk cases: fa_combine_kernel is shared and covered by the F16 suite."""
    return [c for c in R.decode_edge_cases() if c[5] < 512 * R.CHUNK]


def prefill_edge_cases():
    """The ten skip cases, and of the 128-tile segment cases the 8193-key one: the live[] segments are shared code."""
    return [c for c in R.prefill_edge_cases() if c[5] < 8192 or c[5] == 8193]


def type_name(t):
    return T.NAMES[t]
