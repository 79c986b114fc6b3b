"""lfamd_flash_attn on the device (csrc/flash_attn.hip): GGML_OP_FLASH_ATTN_EXT on an F16 K / V cache, both routes.

Every case is built as a -fa graph hands it over: K and V as permuted cache views (memory [token][KV head][D + 8 halves], so
nb1 = n_head_kv * (2 D + 16) and nb2 = 2 D + 16) with the byte 0x7e — a NaN f16 — in every gap and in one whole row behind n_kv; Q with
NaN behind every row; the mask with a row stride beyond 2 n_kv, NaN in the gap and in three rows past n_q; dst pre-filled with a
sentinel.  Checked per case:
  (a) the per-row error of tests/fattn_ref.py against the f64 value on the operands as the route sees them: TOL_F32 (n_q <= 8),
      TOL_MMA (n_q > 8);
  (b) bit equality with calls on one head each;
  (c) every byte outside the D * n_head * n_q * ne3 results unchanged;
  (d) no NaN in the results (a padding lane that read memory, or exp(-inf - -inf), would put one there).
The f64 reference of each case is computed once per case; shapes are fattn_ref's pairwise subsets."""
import numpy as np
import pytest

import fattn_ref as R
from batched_case import NAN32, Dev, span, strided
from llamafile_amd import _hip, ggml_types as T

GAP = 0x7e


@pytest.fixture(scope="module")
def dev(gpu):
    return Dev()


def fill_image(nbytes, view_shape, strides, values, dtype):
    img = np.full(nbytes, GAP, np.uint8)
    strided(img, dtype, view_shape, strides)[...] = values
    return img


def build(Q, K, V, mask, mask_aligned):
    """The byte images and strides (nb3, nb2, nb1) of one case."""
    ne3, n_head, n_q, D = Q.shape
    kvh, n_kv = K.shape[1], K.shape[2]
    q_nb = (n_head * n_q * (4 * D + 16), n_q * (4 * D + 16), 4 * D + 16)
    q_img = np.full(span(Q.shape, q_nb + (4,), 4) // 4 + 4, NAN32, np.uint32)
    strided(q_img, np.uint32, Q.shape, q_nb + (4,))[...] = Q.view(np.uint32)
    row = 2 * D + 16
    kv_nb = ((n_kv + 1) * kvh * row, row, kvh * row)  # one more token row behind n_kv, all NaN
    kv_bytes = ne3 * kv_nb[0]
    k_img = fill_image(kv_bytes, K.shape, kv_nb + (2,), K.view(np.uint16), np.uint16)
    v_img = fill_image(kv_bytes, V.shape, kv_nb + (2,), V.view(np.uint16), np.uint16)
    m_img, m_nb1 = None, 0
    if mask is not None:
        m_nb1 = (2 * n_kv + 2 + 15) // 16 * 16 if mask_aligned else 2 * (n_kv + 3)
        m_img = fill_image((n_q + 3) * m_nb1, mask.shape, (m_nb1, 2), mask.astype(np.float16).view(np.uint16), np.uint16)
    d_nb = (n_q * n_head * (4 * D + 16), 4 * D + 16, n_head * (4 * D + 16))  # (nb3, nb1, nb2): element (i3, j, h, l)
    return q_img, q_nb, k_img, v_img, kv_nb, m_img, m_nb1, d_nb


def sentinel(words):
    return (np.arange(words, dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32) | np.uint32(0x7f800001)


def fa_call(dev, pq, q_nb, pk, pv, kv_nb, pm, m_nb1, D, n_q, n_kv, n_head, kvh, ne3, scale, pd, d_nb, ws=None, expect=0):
    need = dev.lib.lfamd_flash_attn_workspace(D, n_q, n_kv, n_head, kvh, ne3)
    if need and ws is None:
        ws = dev.torch.empty(need, dtype=dev.torch.uint8, device="cuda")
    rc = dev.lib.lfamd_flash_attn(pq, q_nb[2], q_nb[1], q_nb[0], T.F16, pk, kv_nb[2], kv_nb[1], kv_nb[0], T.F16, pv, kv_nb[2], kv_nb[1], kv_nb[0],
                                  pm, m_nb1, D, n_q, n_kv, n_head, kvh, ne3, float(scale), 0.0, pd, d_nb[1], d_nb[2], d_nb[0],
                                  ws.data_ptr() if ws is not None else None, need, 0, None)
    assert rc == expect, _hip.lib().lfamd_last_error()
    return ws


def run_case(dev, case, mask_aligned):
    D, kvh, group, ne3, n_q, n_kv, _, _ = case
    Q, K, V, mask, scale = R.inputs_of(case)
    n_head = kvh * group
    q_img, q_nb, k_img, v_img, kv_nb, m_img, m_nb1, d_nb = build(Q, K, V, mask, mask_aligned)
    dsh, dst_strides = (ne3, n_q, n_head, D), (d_nb[0], d_nb[2], d_nb[1], 4)
    d_img = sentinel(span(dsh, dst_strides, 4) // 4 + 16)
    hq, hk, hv, hd = dev.put(q_img.view(np.uint8), 0), dev.put(k_img, 0), dev.put(v_img, 0), dev.put(d_img.view(np.uint8), 0)
    hm = dev.put(m_img, 0 if mask_aligned else 2) if m_img is not None else None
    pm = dev.ptr(hm) if hm else None
    fa_call(dev, dev.ptr(hq), q_nb, dev.ptr(hk), dev.ptr(hv), kv_nb, pm, m_nb1, D, n_q, n_kv, n_head, kvh, ne3, scale, dev.ptr(hd), d_nb)
    out = dev.get(hd).view(np.uint32).copy()
    got = strided(out, np.uint32, dsh, dst_strides).copy()
    # (c) every byte outside the results is unchanged
    strided(out, np.uint32, dsh, dst_strides)[...] = strided(d_img, np.uint32, dsh, dst_strides)
    assert np.array_equal(out, d_img), "bytes outside the results were written"
    # (d)
    res = got.view(np.float32)
    assert not np.isnan(res).any(), "NaN in the results"
    # (a)
    route = R.route_of(n_q)
    ref, a = R.ref64(Q, K, V, mask, scale, route)
    err = R.row_err(res, ref, a)
    tol = R.TOL_F32 if route == "decode" else R.TOL_MMA
    print(R.case_id(case), route, "err", err, "tol", tol)
    assert err <= tol, (R.case_id(case), err)
    # (b) the same rows by calls on one head each: the same bits
    one = dev.put(np.full(n_q * D * 4, 0xff, np.uint8), 0)
    one_nb = (n_q * D * 4, D * 4, D * 4)  # (nb3, nb1, nb2)
    ws = None
    for i3 in range(ne3):
        for h in range(n_head):
            pq = dev.ptr(hq) + i3 * q_nb[0] + h * q_nb[1]
            off = i3 * kv_nb[0] + (h // group) * kv_nb[1]
            ws = fa_call(dev, pq, q_nb, dev.ptr(hk) + off, dev.ptr(hv) + off, kv_nb, pm, m_nb1, D, n_q, n_kv, 1, 1, 1, scale, dev.ptr(one), one_nb, ws)
            single = dev.get(one).view(np.uint32).reshape(n_q, D)
            assert np.array_equal(single, got[i3, :, h]), ("a row's bits depend on the call's other heads", i3, h)
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("i,case", list(enumerate(R.decode_cases())), ids=lambda v: R.case_id(v) if isinstance(v, tuple) else None)
def test_decode_route(dev, i, case):
    run_case(dev, case, mask_aligned=i % 2 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("i,case", list(enumerate(R.prefill_cases())), ids=lambda v: R.case_id(v) if isinstance(v, tuple) else None)
def test_prefill_route(dev, i, case):
    run_case(dev, case, mask_aligned=i % 2 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_q", [2, 17])
def test_a_misaligned_k_base_is_invalid_and_leaves_dst_untouched(dev, n_q):
    case = (128, 2, 4, 1, n_q, 65, "causal", None)
    Q, K, V, mask, scale = R.inputs_of(case)
    q_img, q_nb, k_img, v_img, kv_nb, m_img, m_nb1, d_nb = build(Q, K, V, mask, True)
    d_img = sentinel(span((1, n_q, 8, 128), (d_nb[0], d_nb[2], d_nb[1], 4), 4) // 4 + 16)
    hq, hk, hv, hd, hm = dev.put(q_img.view(np.uint8), 0), dev.put(k_img, 8), dev.put(v_img, 0), dev.put(d_img.view(np.uint8), 0), dev.put(m_img, 0)
    fa_call(dev, dev.ptr(hq), q_nb, dev.ptr(hk), dev.ptr(hv), kv_nb, dev.ptr(hm), m_nb1, 128, n_q, 65, 8, 2, 1, scale, dev.ptr(hd), d_nb, expect=-2)
    assert np.array_equal(dev.get(hd).view(np.uint32), d_img)
