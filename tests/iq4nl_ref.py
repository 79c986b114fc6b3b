"""NumPy yardstick for IQ4_NL (ggml type 20): the block walk, the dequantisation and the Q8_0 dot product.

A block is {f16 d, uint8 qs[16]} for 32 weights: the low nibble of qs[j] is the codebook index of weight j, the high nibble that of
weight j + 16; weight = d * KVALUES[index].  The CPU oracle (oracle/) does not know the type, so the GPU tests compare against this
file; tests/test_iq4nl_ref.py pins the codebook and checks the two forms of the dot product against each other.
"""
import numpy as np

from llamafile_amd import ggml_types as T, synth

KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], dtype=np.int8)
BLOCK = 18


def _blocks(raw: np.ndarray) -> np.ndarray:
    raw = np.ascontiguousarray(raw)
    assert raw.dtype == np.uint8 and raw.ndim == 2 and raw.shape[1] % BLOCK == 0
    return raw.reshape(raw.shape[0], raw.shape[1] // BLOCK, BLOCK)


def scales(raw: np.ndarray) -> np.ndarray:
    """f32 [rows, blocks]: the blocks' f16 d."""
    return np.ascontiguousarray(_blocks(raw)[:, :, 0:2]).view(np.float16)[..., 0].astype(np.float32)


def codes(raw: np.ndarray) -> np.ndarray:
    """uint8 [rows, blocks, 32]: codebook indices in weight order."""
    qs = _blocks(raw)[:, :, 2:]
    return np.concatenate([qs & 15, qs >> 4], axis=2)


def values(raw: np.ndarray) -> np.ndarray:
    """int8 [rows, blocks, 32]: KVALUES[index]."""
    return KVALUES[codes(raw)]


def dequantize(raw: np.ndarray) -> np.ndarray:
    """f32 [rows, cols]: (d * value) + (+0), one rounding of the product.  The "+ (+0)" is the read-back rule of the 32-block types
    without an m field: under d = -0 a product -0 comes back as +0."""
    with np.errstate(over="ignore", invalid="ignore"):
        w = scales(raw)[:, :, None] * values(raw).astype(np.float32) + np.float32(0.0)
    return w.reshape(raw.shape[0], -1).astype(np.float32)


def _q80(B: np.ndarray):
    B = np.ascontiguousarray(B)
    blk = B.reshape(B.shape[0], B.shape[1] // 34, 34)
    d8 = np.ascontiguousarray(blk[:, :, 0:2]).view(np.float16)[..., 0].astype(np.float32)
    return d8, blk[:, :, 2:].view(np.int8)


def dot_ref(raw: np.ndarray, B: np.ndarray) -> np.ndarray:
    """f64 [n, m]: per 32-block the exact integer sum(value * q8), times f32(f32(d) * f32(d8)), summed in f64.
    B: block_q8_0 rows [n, k/32*34] (synth.quantize_q8_0)."""
    d, v = scales(raw), values(raw).astype(np.float32)
    d8, q8 = _q80(B)
    out = np.zeros((B.shape[0], raw.shape[0]), dtype=np.float64)
    for b in range(d.shape[1]):  # |isum| <= 32 * 127 * 127 < 2^24: every partial sum is an integer f32 holds exactly
        isum = q8[:, b].astype(np.float32) @ v[:, b].T
        with np.errstate(over="ignore", invalid="ignore"):
            s = (d8[:, b][:, None] * d[:, b][None, :]).astype(np.float32)
        out += s.astype(np.float64) * isum.astype(np.float64)
    return out


def dot_dequant(raw: np.ndarray, B: np.ndarray) -> np.ndarray:
    """f64 [n, m]: the other form — dequantise both operands (f32, one rounding each) and multiply in f64."""
    d8, q8 = _q80(B)
    x = (d8[:, :, None] * q8.astype(np.float32)).astype(np.float32).reshape(B.shape[0], -1)
    return x.astype(np.float64) @ dequantize(raw).astype(np.float64).T


def activations(x: np.ndarray) -> np.ndarray:
    """f32 [n, k] -> block_q8_0 rows (tests/test_oracle.py pins this quantiser to the oracle's)."""
    return synth.quantize_q8_0(np.ascontiguousarray(x, dtype=np.float32))


# rows by i % 8, as tests/extremes.py lays its bands out
BAND_MIN, BAND_MAX, BAND_ALT, BAND_BIG = 0, 1, 2, 3
ZERO_ROW = 6  # every block: d = +-0 (the row tests/extremes.py zeroes too)


def extreme_weights(m: int, k: int, seed: int) -> np.ndarray:
    """Raw IQ4_NL rows [m, k/32*18]: bands of all-index-0 (-127) and all-index-15 (113) rows, rows alternating 0 / 15, and in every row
    blocks with negative d, d = 0, d at f16 subnormals (2^-20, either sign) and, in the rows of band 3, d at the largest finite f16
    (65504, either sign); row ZERO_ROW with d = +-0 in every block."""
    raw = synth.random_weights(T.IQ4_NL, m, k, seed).copy()
    blk = _blocks(raw)
    nb = blk.shape[1]
    band = np.arange(m) % 8
    blk[band == BAND_MIN, :, 2:] = 0x00
    blk[band == BAND_MAX, :, 2:] = 0xFF
    blk[band == BAND_ALT, :, 2:] = 0xF0  # weights 0..15 index 0, 16..31 index 15
    blk[band == BAND_ALT, 1::2, 2:] = 0x0F
    d = scales(raw)
    d[:, 1::2] = -d[:, 1::2]
    d[:, 5::7] = 0.0
    d[:, 3::7] = np.float32(2.0 ** -20) * np.where(np.arange(nb)[3::7] % 2, -1, 1)
    big = np.float32(65504.0) * np.where(np.arange(nb)[2::9] % 2, -1, 1)
    d[band == BAND_BIG, 2::9] = big[None, :]
    d[ZERO_ROW] = 0.0
    d[ZERO_ROW, 1::2] = -0.0
    blk[:, :, 0:2] = d.astype(np.float16)[..., None].view(np.uint8)
    return raw
