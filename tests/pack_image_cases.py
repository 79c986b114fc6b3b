"""The cases of tests/golden/pack_images_parent.json and how one is digested: what tools/pack_image_record.py records from a library
built at the parent commit and tests/test_gpu_pack_images.py recomputes with the tree's.  A case is the SHA-256 of the raw GGUF rows,
lfamd_packed_size, and the SHA-256 of the whole output buffer, prefilled with 0xEE, after lfamd_pack_weights; for Q2_K / Q3_K / IQ4_XS
also the outputs of the canonical builder on the raw rows and of the expander on the packed image."""
import ctypes as C
import functools
import hashlib
import json
import os

from llamafile_amd import _hip, ggml_types as T, synth

PAD = _hip.TYPE_PAD256
SEED = 29
TILE_TYPES = (T.Q4_K, T.Q5_K, T.Q6_K, T.Q2_K, T.Q3_K, T.IQ4_XS, T.Q4_0, T.IQ4_NL, T.Q4_1, T.Q5_0, T.Q5_1, T.Q8_0)  # at whole 256-groups
TILE_SHAPES = ((64, 512), (37, 1024), (7, 256))  # partial row tile, one and several super-blocks
BLOCK32 = (T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.IQ4_NL)
BUILDERS = (T.Q2_K, T.Q3_K, T.IQ4_XS)


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_images_parent.json")) as f:
        return json.load(f)


def type_name(t):
    return T.NAMES.get(t & ~PAD, str(t & ~PAD)) + ("|PAD256" if t & PAD else "")


def cases():
    """[(type id, rows, cols)] in the order of the issue's table."""
    out = [(t, r, c) for t in TILE_TYPES for r, c in TILE_SHAPES]
    out += [(T.Q8_0, 7, 96), (T.Q8_0, 37, 160)]  # partial 8-row group, partial quad of blocks
    out += [(t, 37, 288) for t in BLOCK32]  # RAW rows
    out += [(t | PAD, r, c) for t in BLOCK32 for r, c in ((37, 288), (5, 32), (33, 480))]  # kb = 9, 1, 15
    out += [(t, 7, 96) for t in (T.F32, T.F16, T.BF16)]
    return out


def size_only_cases():
    """lfamd_packed_size alone, at the shapes of tests/test_abi_exports.py and tests/test_pad256_abi.py (zeros included)."""
    out = [(t, 4096, 4096) for t in (T.Q4_K, T.Q6_K, T.Q8_0, T.Q2_K, T.Q3_K, T.IQ4_XS, T.Q4_1, T.Q5_0, T.Q5_1)]
    out += [(T.Q8_0, 64, 96), (T.Q4_K, 33, 256), (T.Q4_K, 32, 100), (99, 32, 256)] + [(t, 64, 96) for t in (T.Q4_1, T.Q5_0, T.Q5_1)]
    for t in BLOCK32:
        for rows, cols in ((67, 32), (67, 288), (40, 4000), (4099, 2080)):
            out += [(t | PAD, rows, cols), (t, rows, (cols + 255) // 256 * 256), (t, rows, cols)]
        out += [(u, 67, cols) for cols in (256, 4096) for u in (t, t | PAD)] + [(t | PAD, 67, cols) for cols in (16, 100, 257, 300)]
        out += [(t | PAD, 0, 288), (t | PAD, -1, 288)]
    out += [(t | PAD, 64, 512) for t in (T.Q4_K, T.Q8_0, T.F16, T.F32, T.BF16, T.Q2_K, T.Q3_K, T.Q5_K, T.Q6_K, T.IQ4_XS, 99)]
    out += [(t, 40, c) for t in sorted(T.NAMES) for c in (512, 288)]  # tests/test_gpu_pack.py's stride cases and its type list
    return out


def case_id(t, rows, cols):
    return f"{type_name(t)}-{rows}x{cols}"


def bind(path):
    """A library by path, with the signatures this module calls (the internal launchers are not in _hip._SIGS)."""
    L = C.CDLL(path)
    for name in ("lfamd_init", "lfamd_packed_size", "lfamd_pack_weights", "lfamd_vendor_gemm_available"):
        f = getattr(L, name)
        f.restype, f.argtypes = _hip._SIGS[name]
    vp, sz, lg = C.c_void_p, C.c_size_t, C.c_long
    for name in ("lfamd_wprep16_bytes", "lfamd_wprep8_bytes"):
        getattr(L, name).restype, getattr(L, name).argtypes = sz, [lg, lg]
    for name in ("lfamd_launch_wprep16", "lfamd_launch_wprep8"):
        getattr(L, name).restype, getattr(L, name).argtypes = C.c_int, [C.c_int, vp, sz, lg, lg, vp, vp]
    L.lfamd_launch_pk_expand.restype, L.lfamd_launch_pk_expand.argtypes = C.c_int, [C.c_int, vp, lg, lg, vp, vp]
    L.lfamd_launch_pk4x_expand.restype, L.lfamd_launch_pk4x_expand.argtypes = C.c_int, [vp, lg, lg, vp, vp]
    return L


def packed_size(L, t, rows, cols):
    """lfamd_packed_size without the vendor GEMM's second Q8_0 image (LFAMD_USE_BLASLT=1 adds 2 bytes per weight behind the first)."""
    n = L.lfamd_packed_size(t, rows, cols)
    if t == T.Q8_0 and n and L.lfamd_vendor_gemm_available():
        n -= rows * cols * 2
    return n


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def digest(L, t, rows, cols):
    """One case on the current device.  Q8_0 under LFAMD_USE_BLASLT=1: the digest covers the first image."""
    import torch
    raw = synth.random_weights(t & ~PAD, rows, cols, SEED)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    size, whole = packed_size(L, t, rows, cols), L.lfamd_packed_size(t, rows, cols)
    d_raw = torch.from_numpy(raw).cuda()
    out = torch.full((whole,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = L.lfamd_pack_weights(t, rows, cols, C.c_void_p(d_raw.data_ptr()), raw.shape[1], C.c_void_p(out.data_ptr()), st)
    assert rc == 0, (case_id(t, rows, cols), rc)
    torch.cuda.synchronize()
    rec = {"raw": sha(raw), "size": size, "image": sha(out[:size].cpu().numpy())}
    if t in BUILDERS:
        nbytes = (L.lfamd_wprep8_bytes if t == T.IQ4_XS else L.lfamd_wprep16_bytes)(rows, cols)
        built = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device="cuda")
        expanded = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device="cuda")
        b, e, p = C.c_void_p(built.data_ptr()), C.c_void_p(expanded.data_ptr()), C.c_void_p(out.data_ptr())
        if t == T.IQ4_XS:
            assert L.lfamd_launch_wprep8(t, C.c_void_p(d_raw.data_ptr()), raw.shape[1], rows, cols, b, st) == 0
            assert L.lfamd_launch_pk4x_expand(p, rows, cols, e, st) == 0
        else:
            assert L.lfamd_launch_wprep16(t, C.c_void_p(d_raw.data_ptr()), raw.shape[1], rows, cols, b, st) == 0
            assert L.lfamd_launch_pk_expand(t, p, rows, cols, e, st) == 0
        torch.cuda.synchronize()
        rec.update(canonical_size=nbytes, built=sha(built.cpu().numpy()), expanded=sha(expanded.cpu().numpy()))
    return rec
