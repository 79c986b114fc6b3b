"""The cases of tests/golden/mul_mat_batched_parent.json and how one is digested: what tools/batched_record.py records from a library
built at the parent of the common front end (csrc/mul_mat_batched_common.h) and tests/test_gpu_batched_parent_bits.py recomputes with the
tree's.  A case is the SHA-256 of the A image, of the B image and of the WHOLE result buffer — prefilled with tests/batched_case.py's
sentinel — after the call, so a write outside the results moves the digest as a wrong bit inside them does.

The list reaches every kernel instantiation of the two launchers (48; kernels_reached() names them as the library's symbols do):
  F16 GEMV   {16, 64} lanes (k <= 128, k > 128) x NC {1, 2, 4, 8} x {aligned, unaligned};  F16 MFMA {aligned, unaligned};
  block-K GEMV  six types x NC {1, 2, 4, 8};  block-K MFMA  six types
and every branch of the host side: a chunked group (r2 = 3, n = 3: hg = 2, hchunks = 2, the last chunk of one head), an ne3 broadcast,
row counts that leave a partial work-group, an MFMA wave without its second row tile (m = 130: the wave at row 128), k / 32 not a
multiple of 4 (k = 160), and the batch body's dynamic LDS above 64 KiB (k = 1024, n = 16; Q8_0 and Q4_1).  Shapes are the smallest
that do this: m <= 130, n <= 65, at most 8 slices."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np

from llamafile_amd import _hip, ggml_types as T, synth
import batched_case as bc

SEED = 31
SIX = (T.Q8_0, T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.IQ4_NL)
# (n, r2) whose hg * n = min(r2, 8 / n) * n is 1, 2, 4 and 6: NC = 1, 2, 4, 8; the last one is the chunked group
NC_SHAPES = {1: (1, 1), 2: (2, 1), 4: (1, 4), 8: (3, 3)}


def case(t, m, k, n, kvh, group, ne3=1, a_ne3=1, unaligned=False):
    return (t, m, k, n, kvh, group, ne3, a_ne3, unaligned)


def cases():
    out = []
    for nc, (n, group) in NC_SHAPES.items():
        for k in (128, 136):  # 16 lanes; 64 lanes with a k tail (rows of 136 halves lie on 16 bytes)
            for unaligned in (False, True):
                out.append(case(T.F16, 70 if k == 128 else 6, k, n, 2, group, unaligned=unaligned))  # (64 + 6 rows; 4 + 2 rows)
        for t in SIX:
            out.append(case(t, 70, 160, n, 2, group, unaligned=nc == 2))  # five blocks: a quad's round and one lane of a second
    for unaligned in (False, True):
        out.append(case(T.F16, 130, 72, 9, 1, 2, ne3=2, a_ne3=1, unaligned=unaligned))  # ne3 broadcast; a wave with one row tile
    for t in SIX:
        out.append(case(t, 130, 160, 65, 1, 2, ne3=2, a_ne3=1, unaligned=t == T.Q5_0))  # a second column tile of one column
    out += [case(t, 40, 1024, 16, 1, 1) for t in (T.Q8_0, T.Q4_1)]
    out.append(case(T.Q5_1, 33, 32, 5, 1, 3, ne3=2, a_ne3=2))  # one block; hg = 1 < r2; ne3 = a_ne3 = 2
    return out


def case_id(c):
    t, m, k, n, kvh, group, ne3, a_ne3, unaligned = c
    return f"{T.NAMES[t]}-m{m}k{k}n{n}-kv{kvh}x{group}-ne3_{ne3}of{a_ne3}" + ("-unaligned" if unaligned else "")


def entry_point(t):
    return "lfamd_mul_mat_batched" if t == T.F16 else "lfamd_mul_mat_batched_q"


def kernels_reached(c):
    """The kernel the launchers pick for a case, written as a fragment of its mangled name (template arguments as Itanium spells
    them: Li<N>E an int, Lb<0|1>E a bool)."""
    t, m, k, n, kvh, group, ne3, a_ne3, unaligned = c
    nc_max = min(group, 8 // n) * n if n <= 8 else 0
    nc = next((v for v in (1, 2, 4, 8) if nc_max <= v), None)
    if t == T.F16:
        al = f"Lb{0 if unaligned else 1}E"
        return f"mmb_gemv_kernelILi{16 if k <= 128 else 64}ELi{nc}E{al}E" if n <= 8 else f"mmb_mfma_kernelI{al}E"
    return f"mmq_gemv_kernelILi{t}ELi{nc}EE" if n <= 8 else f"mmq_mfma_kernelILi{t}EE"


def layout(row, m, k, n, kvh, heads, unaligned):
    """Byte strides (nb3, nb2, nb1) of A (rows of `row` bytes), B and C.  Default: the permuted K cache — A memory [m][kv head][row and a
    gap, on 16 bytes], B memory [n][head][k + 4 floats].  unaligned: a_nb1 = row + 2 (A memory [kv head][m]), b_nb1 = (k + 1) * 4,
    c_nb1 = (m + 1) * 4, and batched_case puts the bases off 16 bytes.  C has padded rows and one padded row per slice."""
    if unaligned:
        a1, b1, c1 = row + 2, (k + 1) * 4, (m + 1) * 4
        a, b = (kvh * m * a1, m * a1, a1), (heads * n * b1, n * b1, b1)
    else:
        a2, b2, c1 = (row + 31) // 16 * 16, (k + 4) * 4, (m + 3) * 4
        a, b = (m * kvh * a2, a2, kvh * a2), (n * heads * b2, b2, heads * b2)
    return a, b, (heads * (n + 1) * c1 + 8, (n + 1) * c1, c1)


def images(c):
    """(A image uint8, B image uint32, dims, a_nb, b_nb, c_nb) of a case, from SEED alone.  Gaps: 0x7e bytes in A (a NaN as f16 and as
    a block's d), NaN in B."""
    t, m, k, n, kvh, group, ne3, a_ne3, unaligned = c
    heads, row = kvh * group, T.row_size(t, k)
    a_nb, b_nb, c_nb = layout(row, m, k, n, kvh, heads, unaligned)
    seed = SEED + 1000 * cases().index(c)
    Av = synth.random_weights(t, a_ne3 * kvh * m, k, seed).reshape(a_ne3, kvh, m, row)
    Bv = synth.random_activations(ne3 * heads * n, k, seed + 1).reshape(ne3, heads, n, k)
    A_img = np.full(bc.span(Av.shape, a_nb + (1,), 1) + 6, 0x7e, np.uint8)
    bc.strided(A_img, np.uint8, Av.shape, a_nb + (1,))[...] = Av
    return A_img, bc.b_image(Bv, b_nb, 4), (m, k, n, kvh, a_ne3, heads, ne3), a_nb, b_nb, c_nb


def bind(path):
    """A library by path, with the signatures of the two calls."""
    L = C.CDLL(path)
    for name in ("lfamd_init", "lfamd_last_error", "lfamd_mul_mat_batched", "lfamd_mul_mat_batched_q"):
        f = getattr(L, name)
        f.restype, f.argtypes = _hip._SIGS[name]
    return L


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def digest(dev, L, c):
    """One case on the current device with the library L."""
    A_img, B_img, dims, a_nb, b_nb, c_nb = images(c)
    fn = getattr(L, entry_point(c[0]))
    _, _, _, out = bc.call_on_images(dev, fn, c[0], A_img, B_img, dims, a_nb, b_nb, c_nb, c[-1])
    return {"A": sha(A_img), "B": sha(B_img), "C": sha(out)}


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mul_mat_batched_parent.json")) as f:
        return json.load(f)
