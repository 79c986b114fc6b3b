"""The argument-check cases of lfamd_flash_attn and lfamd_cpy (include/lfamd_hip.h, "Checks, before any device call and in this
order"), shared by tests/test_entry_checks.py and tools/entry_checks_record.py: per operator a control call that passes every check,
and named changes to it.  A case is (name, expectation, changes); the expectation is the author's reading of the header:
    REFUSED  a check answers with an error code and a message, before any device call
    EMPTY    LFAMD_OK, nothing launched
    PASSES   every check passes — such a call reaches the device, so it is NEVER sent to an entry point with these made-up
             addresses, only to the check functions
No device memory stands behind the addresses: they are numbers with the alignment the operands need."""
import ctypes as C

from llamafile_amd import _hip, ggml_types as T

REFUSED, EMPTY, PASSES = "refused", "empty", "passes"
CHECK_UNPLACED = _hip.CHECK_UNPLACED
ERR_UNSUPPORTED, ERR_INVALID, ERR_HIP, ERR_WORKSPACE = -1, -2, -3, -4

Q_AT, K_AT, V_AT, MASK_AT, DST_AT, WS_AT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000
SRC_AT = 0x10000000

# ---- lfamd_flash_attn.  The control: tests/backend_host/fattn_host.c's layouts (Q memory [n_q][heads][D], K / V the permuted cache
# views [n_kv][kv heads][D], dst contiguous [D, n_head, n_q]) at D 128, one query, six keys, 8 heads on 2 KV heads, ne3 1
D, N_Q, N_KV, HEADS, KVH = 128, 1, 6, 8, 2
FA_ARGS = ("Q", "q_nb1", "q_nb2", "q_nb3", "Ktype", "K", "k_nb1", "k_nb2", "k_nb3", "Vtype", "V", "v_nb1", "v_nb2", "v_nb3", "mask", "mask_nb1",
           "D", "n_q", "n_kv", "n_head", "n_head_kv", "ne3", "scale", "max_bias", "dst", "dst_nb1", "dst_nb2", "dst_nb3", "ws", "ws_bytes",
           "flags", "stream")
FA_CONTROL = dict(Q=Q_AT, q_nb1=HEADS * D * 4, q_nb2=D * 4, q_nb3=N_Q * HEADS * D * 4, Ktype=T.F16, K=K_AT, k_nb1=KVH * D * 2, k_nb2=D * 2,
                  k_nb3=N_KV * KVH * D * 2, Vtype=T.F16, V=V_AT, v_nb1=KVH * D * 2, v_nb2=D * 2, v_nb3=N_KV * KVH * D * 2, mask=MASK_AT,
                  mask_nb1=N_KV * 2, D=D, n_q=N_Q, n_kv=N_KV, n_head=HEADS, n_head_kv=KVH, ne3=1, scale=D ** -0.5, max_bias=0.0, dst=DST_AT,
                  dst_nb1=D * 4, dst_nb2=HEADS * D * 4, dst_nb3=N_Q * HEADS * D * 4, ws=None, ws_bytes=0, flags=0, stream=None)
NO_POINTERS = dict(Q=None, K=None, V=None, mask=None, dst=None, ws=None)
# 600 keys under one query: the split route, three chunks of 256 -> ne3 * n_head * n_q * 3 * (D + 2) * 4 bytes of workspace
LONG = dict(n_kv=600, k_nb3=600 * KVH * D * 2, v_nb3=600 * KVH * D * 2, mask_nb1=1200)
LONG_WS = 1 * HEADS * 1 * 3 * (D + 2) * 4
SHORT_WS = dict(LONG, ws=WS_AT, ws_bytes=LONG_WS - 1)

FA_CASES = [
    ("control", PASSES, {}),
    ("control_nomask", PASSES, dict(mask=None, mask_nb1=0)),
    ("control_long_with_its_workspace", PASSES, dict(LONG, ws=WS_AT, ws_bytes=LONG_WS)),
    # step 1
    ("negative_D", REFUSED, dict(D=-128)),
    ("negative_ne3", REFUSED, dict(ne3=-1)),
    # step 2: nothing else is looked at
    ("n_q_0", EMPTY, dict(NO_POINTERS, n_q=0, Ktype=T.Q4_0)),
    ("n_head_0", EMPTY, dict(NO_POINTERS, n_head=0, Ktype=T.Q4_0)),
    ("ne3_0", EMPTY, dict(NO_POINTERS, ne3=0, Ktype=T.Q4_0)),
    # step 3, clause by clause
    ("k_q4_0", REFUSED, dict(Ktype=T.Q4_0)),
    ("v_f32", REFUSED, dict(Vtype=T.F32)),
    ("d96", REFUSED, dict(D=96)),
    ("max_bias_1", REFUSED, dict(max_bias=1.0)),
    ("heads_256_ne3_256", REFUSED, dict(n_head=256, ne3=256)),
    ("n_q_query_blocks", REFUSED, dict(n_q=128 * 65535 + 1)),
    ("n_kv_0", REFUSED, dict(n_kv=0)),
    # step 4, clause by clause
    ("null_Q", REFUSED, dict(Q=None)),
    ("null_K", REFUSED, dict(K=None)),
    ("null_V", REFUSED, dict(V=None)),
    ("null_dst", REFUSED, dict(dst=None)),
    ("null_workspace_with_a_size", REFUSED, dict(ws=None, ws_bytes=16)),
    ("n_head_kv_0", REFUSED, dict(n_head_kv=0)),
    ("n_head_kv_3", REFUSED, dict(n_head_kv=3)),
    ("k_base_plus_8", REFUSED, dict(K=K_AT + 8)),
    ("q_nb2_plus_8", REFUSED, dict(q_nb2=D * 4 + 8)),
    ("dst_nb3_plus_8", REFUSED, dict(dst_nb3=N_Q * HEADS * D * 4 + 8)),
    ("v_nb1_8", REFUSED, dict(v_nb1=8)),
    ("mask_base_plus_1", REFUSED, dict(mask=MASK_AT + 1)),
    ("mask_nb1_plus_1", REFUSED, dict(mask_nb1=N_KV * 2 + 1)),
    ("mask_nb1_short", REFUSED, dict(mask_nb1=N_KV * 2 - 2)),
    ("k_nb1_short", REFUSED, dict(k_nb1=D * 2 - 16)),
    ("v_nb1_short", REFUSED, dict(v_nb1=D * 2 - 16)),
    ("q_nb1_short", REFUSED, dict(q_nb1=D * 4 - 16)),
    ("dst_nb1_short", REFUSED, dict(dst_nb1=D * 4 - 16)),
    ("flags_1", REFUSED, dict(flags=1)),
    # step 5
    ("workspace_one_byte_short", REFUSED, SHORT_WS),
    # two consecutive steps violated: the earlier one answers
    ("steps_1_2_negative_D_and_n_q_0", REFUSED, dict(D=-128, n_q=0)),
    ("steps_2_3_ne3_0_and_d96", EMPTY, dict(ne3=0, D=96)),
    ("steps_3_4_d96_and_null_Q", REFUSED, dict(D=96, Q=None)),
    ("steps_4_5_flags_1_and_short_workspace", REFUSED, dict(SHORT_WS, flags=1)),
    # two clauses of one step: the documented order inside it
    ("step_3_k_q4_0_before_d96", REFUSED, dict(Ktype=T.Q4_0, D=96)),
    ("step_3_d96_before_max_bias", REFUSED, dict(D=96, max_bias=1.0)),
    ("step_3_max_bias_before_slices", REFUSED, dict(max_bias=1.0, n_head=256, ne3=256)),
    ("step_3_slices_before_n_kv_0", REFUSED, dict(n_head=256, ne3=256, n_kv=0)),
    ("step_4_null_before_n_head_kv", REFUSED, dict(V=None, n_head_kv=3)),
    ("step_4_n_head_kv_before_alignment", REFUSED, dict(n_head_kv=3, K=K_AT + 8)),
    ("step_4_alignment_before_mask", REFUSED, dict(K=K_AT + 8, mask=MASK_AT + 1)),
    ("step_4_mask_before_row_strides", REFUSED, dict(mask_nb1=N_KV * 2 - 2, q_nb1=D * 4 - 16)),
    ("step_4_row_strides_before_flags", REFUSED, dict(q_nb1=D * 4 - 16, flags=1)),
]

# under LFAMD_CHECK_UNPLACED (the check functions only): (name, changes, the recorded case whose answer it must give, or None: LFAMD_OK)
FA_UNPLACED = [
    ("every_pointer_null", NO_POINTERS, None),
    ("k_pointer_8", dict(NO_POINTERS, K=8), "k_base_plus_8"),
    ("workspace_one_byte_short", SHORT_WS, None),
    ("null_workspace_with_a_size", dict(ws=None, ws_bytes=16), None),
    ("d96", dict(NO_POINTERS, D=96), "d96"),
    ("q_nb1_short", dict(NO_POINTERS, q_nb1=D * 4 - 16), "q_nb1_short"),
    ("flags_1_beside_it", dict(flags=1), "flags_1"),
]

# ---- lfamd_cpy.  The control: tests/backend_host/cpy_host.c's K store, F32 [128, 2, 3] into a Q8_0 1-D view of 768 elements
CPY_ARGS = ("src_type", "src", "src_ne", "src_nb", "dst_type", "dst", "dst_ne", "dst_nb", "flags", "stream")
ROW80 = 768 // 32 * 34
CPY_CONTROL = dict(src_type=T.F32, src=SRC_AT, src_ne=(128, 2, 3, 1), src_nb=(4, 512, 1024, 3072), dst_type=T.Q8_0, dst=K_AT + 5 * 272,
                   dst_ne=(768, 1, 1, 1), dst_nb=(34, ROW80, ROW80, ROW80), flags=0, stream=None)
F16_DST = dict(dst_type=T.F16, dst_nb=(2, 1536, 1536, 1536))  # control_f16: the same source into an F16 view
F32_ROWS = dict(src_ne=(128, 6, 1, 1), src_nb=(4, 512, 3072, 3072))
TWO_31 = dict(ne=(65536, 32768, 1, 1), nb=(4, 262144, 1 << 33, 1 << 33))  # 2^31 F32 elements

CPY_CASES = [
    ("control", PASSES, {}),
    ("control_f16", PASSES, F16_DST),
    ("control_move", PASSES, dict(src_type=T.Q8_0, src_ne=(768, 1, 1, 1), src_nb=(34, ROW80, ROW80, ROW80))),
    # step 1
    ("null_src_ne", REFUSED, dict(src_ne=None)),
    ("null_src_nb", REFUSED, dict(src_nb=None)),
    ("null_dst_ne", REFUSED, dict(dst_ne=None)),
    ("null_dst_nb", REFUSED, dict(dst_nb=None)),
    ("negative_src_extent", REFUSED, dict(src_ne=(128, 2, -3, 1))),
    ("negative_dst_extent", REFUSED, dict(dst_ne=(768, 1, 1, -1))),
    # step 2: no pointer, type or stride is looked at
    ("dst_zero_extent_bad_types", EMPTY, dict(dst_ne=(768, 0, 1, 1), src_type=T.Q6_K, dst_type=T.BF16, src=None, dst=None, dst_nb=(3, 5, 7, 9))),
    # step 3
    ("f16_to_f32", REFUSED, dict(src_type=T.F16, dst_type=T.F32)),
    ("f32_to_q6_k", REFUSED, dict(dst_type=T.Q6_K)),
    ("src_2_31_elements", REFUSED, dict(dst_type=T.F32, src_ne=TWO_31["ne"], src_nb=TWO_31["nb"], dst_ne=(768, 1, 1, 1), dst_nb=(4, 3072, 3072, 3072))),
    ("dst_2_31_elements", REFUSED, dict(dst_type=T.F32, dst_ne=TWO_31["ne"], dst_nb=TWO_31["nb"])),
    # step 4, clause by clause
    ("null_src", REFUSED, dict(src=None)),
    ("null_dst", REFUSED, dict(dst=None)),
    ("unequal_counts", REFUSED, dict(dst_ne=(736, 1, 1, 1))),
    ("src_ne0_48", REFUSED, dict(src_ne=(48, 16, 1, 1), src_nb=(4, 192, 3072, 3072))),
    ("dst_ne0_48", REFUSED, dict(dst_ne=(48, 16, 1, 1))),
    ("dst_nb0_36", REFUSED, dict(dst_nb=(36, ROW80, ROW80, ROW80))),
    ("src_nb0_8", REFUSED, dict(src_nb=(8, 1024, 2048, 6144))),
    ("f16_base_odd", REFUSED, dict(F16_DST, dst=K_AT + 1)),
    ("q8_0_base_odd", REFUSED, dict(dst=K_AT + 5 * 272 + 1)),
    ("f32_stride_6", REFUSED, dict(F16_DST, src_nb=(4, 512, 1024, 6))),
    ("f32_base_plus_2", REFUSED, dict(src=SRC_AT + 2)),
    ("src_row_stride_short", REFUSED, {**F16_DST, **F32_ROWS, "src_nb": (4, 256, 3072, 3072)}),
    ("dst_row_stride_short", REFUSED, dict(F32_ROWS, dst_type=T.F16, dst_ne=(128, 6, 1, 1), dst_nb=(2, 128, 1536, 1536))),
    ("flags_1", REFUSED, dict(flags=1)),
    # two consecutive steps violated: the earlier one answers
    ("steps_1_2_negative_src_extent_and_zero_dst_extent", REFUSED, dict(src_ne=(128, 2, -3, 1), dst_ne=(768, 0, 1, 1))),
    ("steps_2_3_zero_dst_extent_and_f16_to_f32", EMPTY, dict(dst_ne=(768, 0, 1, 1), src_type=T.F16, dst_type=T.F32)),
    ("steps_3_4_f16_to_f32_and_null_src", REFUSED, dict(src_type=T.F16, dst_type=T.F32, src=None)),
    # two clauses of one step: the documented order inside it
    ("step_1_null_array_before_negative_extent", REFUSED, dict(dst_nb=None, src_ne=(128, 2, -3, 1))),
    ("step_3_type_pair_before_element_limit", REFUSED, dict(dst_type=T.Q6_K, dst_ne=TWO_31["ne"])),
    ("step_4_null_before_unequal_counts", REFUSED, dict(src=None, dst_ne=(736, 1, 1, 1))),
    ("step_4_unequal_counts_before_ne0", REFUSED, dict(dst_ne=(752, 1, 1, 1))),
    ("step_4_ne0_before_nb0", REFUSED, dict(src_ne=(48, 16, 1, 1), dst_nb=(36, ROW80, ROW80, ROW80))),
    ("step_4_nb0_before_alignment", REFUSED, dict(dst_nb=(36, ROW80, ROW80, ROW80), src=SRC_AT + 2)),
    ("step_4_alignment_before_row_stride", REFUSED, {**F16_DST, **F32_ROWS, "src_nb": (4, 254, 3072, 3072)}),
    ("step_4_row_stride_before_flags", REFUSED, {**F16_DST, **F32_ROWS, "src_nb": (4, 256, 3072, 3072), "flags": 1}),
]

CPY_UNPLACED = [
    ("every_pointer_null", dict(src=None, dst=None), None),
    ("dst_pointer_1", dict(src=None, dst=1), "q8_0_base_odd"),
    ("f32_to_q6_k", dict(src=None, dst=None, dst_type=T.Q6_K), "f32_to_q6_k"),
    ("src_row_stride_short", {**F16_DST, **F32_ROWS, "src_nb": (4, 256, 3072, 3072), "src": None, "dst": None}, "src_row_stride_short"),
    ("flags_1_beside_it", dict(flags=1), "flags_1"),
]

OPERATORS = {"lfamd_flash_attn": (FA_ARGS, FA_CONTROL, FA_CASES, FA_UNPLACED), "lfamd_cpy": (CPY_ARGS, CPY_CONTROL, CPY_CASES, CPY_UNPLACED)}
NOT_IN_CHECK = {"lfamd_flash_attn": ("scale", "stream"), "lfamd_cpy": ("stream",)}  # what the check functions' argument lists leave out

_vp, _sz, _l, _i, _u, _f = C.c_void_p, C.c_size_t, C.c_long, C.c_int, C.c_uint, C.c_float
_FA_TYPES = dict(Q=_vp, K=_vp, V=_vp, mask=_vp, dst=_vp, ws=_vp, stream=_vp, Ktype=_i, Vtype=_i, scale=_f, max_bias=_f, flags=_u,
                 D=_l, n_q=_l, n_kv=_l, n_head=_l, n_head_kv=_l, ne3=_l)
_CPY_TYPES = dict(src_type=_i, dst_type=_i, src=_vp, dst=_vp, stream=_vp, flags=_u, src_ne=C.POINTER(_l), dst_ne=C.POINTER(_l),
                  src_nb=C.POINTER(_sz), dst_nb=C.POINTER(_sz))


def _ctype(op, name):
    return (_FA_TYPES if op == "lfamd_flash_attn" else _CPY_TYPES).get(name, _sz)


def bind(path):
    """The library at `path` with the entry points' signatures, and the check functions' where it has them."""
    import torch  # noqa: F401  (first: its HIP runtime is the one the library must resolve to, as in llamafile_amd/_hip.py)
    lib = C.CDLL(path)
    lib.lfamd_last_error.restype = C.c_char_p
    for op, (names, _, _, _) in OPERATORS.items():
        getattr(lib, op).argtypes = [_ctype(op, n) for n in names]
        if hasattr(lib, op + "_check"):
            getattr(lib, op + "_check").argtypes = [_ctype(op, n) for n in names if n not in NOT_IN_CHECK[op]]
    return lib


def arguments(op, changes, check, flags=0):
    """The control's argument list with `changes`, for the entry point or (check) its check function; `flags` is OR-ed in."""
    names, control, _, _ = OPERATORS[op]
    a = dict(control, **changes)
    a["flags"] |= flags
    out = []
    for n in names:
        if check and n in NOT_IN_CHECK[op]:
            continue
        v = a[n]
        if isinstance(v, tuple):  # ne / nb: a host array of four
            v = ((_l if n.endswith("_ne") else _sz) * 4)(*v)
        out.append(v)
    return out


def call(lib, op, changes, check, flags=0):
    """(rc, message): the message is what lfamd_last_error() holds after a non-zero answer, "" after LFAMD_OK."""
    rc = getattr(lib, op + ("_check" if check else ""))(*arguments(op, changes, check, flags))
    return rc, (lib.lfamd_last_error().decode() if rc else "")
