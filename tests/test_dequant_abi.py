"""CPU-side checks of the weight read-back calls (lfamd_get_rows, lfamd_unpack_weights): the ABI carries them, and the yardstick
the GPU tests compare against (oracle.c: ora_dequantize_row) is pinned to a NumPy restatement written here from
include/lfamd_blocks.h, so tests/test_gpu_get_rows.py cannot pass against a drifting definition.

Operation order, all in f32, one rounding per operation:  K-quants ((d * sc) * q) - (dmin * mn);  32-blocks (d * q) + m."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T, synth
import extremes
import pack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lfamd_get_rows", "lfamd_unpack_weights")
ROWS, COLS = 67, 1024


def test_read_back_calls_are_exported_declared_and_bound():
    assert os.path.exists(_hip.HIP_SO), "run __graft_entry__.build() first"
    lib = C.CDLL(_hip.HIP_SO)
    hdr = open(os.path.join(ROOT, "include", "lfamd_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the HIP module"
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/lfamd_hip.h"
        assert name in _hip.EXPORTS
    assert lib.lfamd_abi_version() == 1  # additions only


def _f16(blk, off):
    return np.ascontiguousarray(blk[..., off:off + 2]).view(np.float16)[..., 0].astype(np.float32)


def _scale_min_k4(sc12):
    """get_scale_min_k4 on all eight sub-blocks: scales[12] -> (sc[8], mn[8])."""
    q = sc12.astype(np.int32)
    sc = np.empty(q.shape[:-1] + (8,), np.int32)
    mn = np.empty_like(sc)
    sc[..., :4] = q[..., 0:4] & 63
    mn[..., :4] = q[..., 4:8] & 63
    sc[..., 4:] = (q[..., 8:12] & 0xF) | ((q[..., 0:4] >> 6) << 4)
    mn[..., 4:] = (q[..., 8:12] >> 4) | ((q[..., 4:8] >> 6) << 4)
    return sc, mn


def np_dequantize(t, raw, cols):
    rows = raw.shape[0]
    f = np.float32
    if t == T.Q4_K:
        nb = cols // 256
        codes, hdr = pack_ref.q4k_codes(raw, nb)
        d, dmin = _f16(hdr, 0), _f16(hdr, 2)
        sc, mn = _scale_min_k4(hdr[..., 4:16])
        q = codes.reshape(rows, nb, 8, 32).astype(f)
        dl = d[..., None] * sc.astype(f)
        ml = dmin[..., None] * mn.astype(f)
        return ((dl[..., None] * q) - ml[..., None]).reshape(rows, cols)
    if t == T.Q6_K:
        nb = cols // 256
        codes, sc, dd = pack_ref.q6k_codes(raw, nb)
        d = _f16(dd, 0)
        q = (codes.astype(np.int32) - 32).reshape(rows, nb, 16, 16).astype(f)
        dl = d[..., None] * sc.view(np.int8).astype(f)
        return ((dl[..., None] * q) - f(0.0) * f(0.0)).reshape(rows, cols)
    blk = raw.reshape(rows, cols // 32, T.TYPE_SIZE[t])
    d = _f16(blk, 0)
    if t == T.Q8_0:
        q = blk[..., 2:].view(np.int8).astype(f)
    elif t == T.Q4_0:
        qs = blk[..., 2:].astype(np.int32)
        q = np.concatenate([(qs & 15) - 8, (qs >> 4) - 8], axis=-1).astype(f)
    else:
        raise AssertionError(t)
    return ((d[..., None] * q) + f(0.0)).reshape(rows, cols)


@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("t", [T.Q4_K, T.Q6_K, T.Q8_0, T.Q4_0], ids=lambda t: T.NAMES[t])
def test_oracle_dequantize_is_the_stated_arithmetic(oracle, t, gen):
    raw = synth.random_weights(t, ROWS, COLS, 5) if gen == "plain" else extremes.extreme_weights(t, ROWS, COLS, 5)
    want = np.ascontiguousarray(np_dequantize(t, raw, COLS), dtype=np.float32)
    got = oracle.dequantize(t, raw, COLS)
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{T.NAMES[t]} {gen}: {diff} of {got.size} words differ")
    assert diff == 0


def test_generators_exercise_sign_of_zero_and_f16_subnormals(oracle):
    """Bit comparison only tests operation order, the sign of zero and subnormal rounding if the inputs produce them."""
    negz = sub = 0
    for t in T.QUANT_WEIGHT_TYPES:
        for gen in ("plain", "extreme"):
            raw = synth.random_weights(t, ROWS, COLS, 5) if gen == "plain" else extremes.extreme_weights(t, ROWS, COLS, 5)
            w = oracle.dequantize(t, raw, COLS)
            assert np.isfinite(w).all(), (T.NAMES[t], gen)
            h = w.astype(np.float16)
            assert np.isfinite(h).all(), (T.NAMES[t], gen)  # no F16 overflow on these inputs
            nz = int((w.view(np.uint32) == 0x80000000).sum())
            sn = int(((h != 0) & (np.abs(h.astype(np.float32)) < 2.0 ** -14)).sum())
            print(f"{T.NAMES[t]} {gen}: {nz} negative zeros, {sn} f16 subnormals")
            negz += nz
            sub += sn
    assert negz > 0 and sub > 0
