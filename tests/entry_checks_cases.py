"""The argument-check cases of lfamd_flash_attn, lfamd_flash_attn_q, lfamd_cpy, lfamd_mul_mat_batched and lfamd_mul_mat_batched_q
(include/lfamd_hip.h, "Checks, before any device call and in this order"), shared by tests/test_entry_checks.py and
tools/entry_checks_record.py: per operator a control call that passes every check, and named changes to it.  A case is (name, expectation, changes); the expectation is the author's reading of the header:
    REFUSED  a check answers with an error code and a message, before any device call
    EMPTY    LFAMD_OK, nothing launched
    PASSES   every check passes — such a call reaches the device, so it is NEVER sent to an entry point with these made-up
             addresses, only to the check functions
             (the two batched calls have no check function: their PASSES rows document the control and are sent nowhere; that a
             row does NOT answer is shown by a refused call whose later row answers instead)
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

# ---- lfamd_flash_attn_q: lfamd_flash_attn's argument list and control on a Q8_0 cache (rows of D / 32 blocks of 34 bytes; Q4_0: 18)
ROW_Q80, ROW_Q40 = D // 32 * 34, D // 32 * 18
FAQ_CONTROL = dict(FA_CONTROL, Ktype=T.Q8_0, k_nb1=KVH * ROW_Q80, k_nb2=ROW_Q80, k_nb3=N_KV * KVH * ROW_Q80, Vtype=T.Q8_0, v_nb1=KVH * ROW_Q80,
                   v_nb2=ROW_Q80, v_nb3=N_KV * KVH * ROW_Q80)
Q40_PAIR = dict(Ktype=T.Q4_0, k_nb1=KVH * ROW_Q40, k_nb2=ROW_Q40, k_nb3=N_KV * KVH * ROW_Q40, Vtype=T.Q4_0, v_nb1=KVH * ROW_Q40, v_nb2=ROW_Q40,
                v_nb3=N_KV * KVH * ROW_Q40)
F16_PAIR = {n: FA_CONTROL[n] for n in Q40_PAIR}
FAQ_LONG = dict(n_kv=600, k_nb3=600 * KVH * ROW_Q80, v_nb3=600 * KVH * ROW_Q80, mask_nb1=1200)
FAQ_SHORT_WS = dict(FAQ_LONG, ws=WS_AT, ws_bytes=LONG_WS - 1)

FAQ_CASES = [
    ("control", PASSES, {}),
    ("control_q4_0", PASSES, Q40_PAIR),
    ("control_nomask", PASSES, dict(mask=None, mask_nb1=0)),
    ("control_long_with_its_workspace", PASSES, dict(FAQ_LONG, ws=WS_AT, ws_bytes=LONG_WS)),
    ("k_base_plus_2", PASSES, dict(K=K_AT + 2)),  # a block lies on a 2-byte boundary and no better
    ("v_nb3_plus_2", PASSES, dict(v_nb3=N_KV * KVH * ROW_Q80 + 2)),
    ("q4_0_rows_of_72", PASSES, dict(Q40_PAIR, k_nb1=ROW_Q40, v_nb1=ROW_Q40)),
    # step 1
    ("negative_D", REFUSED, dict(D=-128)),
    ("negative_n_head_kv", REFUSED, dict(n_head_kv=-2)),
    # step 2: nothing else is looked at
    ("n_q_0", EMPTY, dict(NO_POINTERS, n_q=0, Ktype=T.F16)),
    ("n_head_0", EMPTY, dict(NO_POINTERS, n_head=0, Vtype=T.Q6_K)),
    ("ne3_0", EMPTY, dict(NO_POINTERS, ne3=0, flags=1)),
    # step 3: the pair rule, then lfamd_flash_attn's clauses
    ("f16_pair", REFUSED, F16_PAIR),
    ("k_q8_0_v_q4_0", REFUSED, dict(Vtype=T.Q4_0)),
    ("k_q4_0_v_q8_0", REFUSED, dict(Ktype=T.Q4_0)),
    ("k_q8_0_v_f16", REFUSED, dict(Vtype=T.F16)),
    ("k_f16_v_q8_0", REFUSED, dict(Ktype=T.F16)),
    ("q4_1_pair", REFUSED, dict(Ktype=T.Q4_1, Vtype=T.Q4_1)),
    ("q5_0_pair", REFUSED, dict(Ktype=T.Q5_0, Vtype=T.Q5_0)),
    ("iq4_nl_pair", REFUSED, dict(Ktype=T.IQ4_NL, Vtype=T.IQ4_NL)),
    ("q4_k_pair", REFUSED, dict(Ktype=T.Q4_K, Vtype=T.Q4_K)),
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
    ("q_base_plus_8", REFUSED, dict(Q=Q_AT + 8)),
    ("q_nb2_plus_8", REFUSED, dict(q_nb2=D * 4 + 8)),
    ("dst_nb3_plus_8", REFUSED, dict(dst_nb3=N_Q * HEADS * D * 4 + 8)),
    ("k_base_plus_1", REFUSED, dict(K=K_AT + 1)),
    ("k_nb2_plus_1", REFUSED, dict(k_nb2=ROW_Q80 + 1)),
    ("v_base_plus_1", REFUSED, dict(V=V_AT + 1)),
    ("v_nb1_plus_1", REFUSED, dict(v_nb1=KVH * ROW_Q80 + 1)),
    ("mask_base_plus_1", REFUSED, dict(mask=MASK_AT + 1)),
    ("mask_nb1_plus_1", REFUSED, dict(mask_nb1=N_KV * 2 + 1)),
    ("mask_nb1_short", REFUSED, dict(mask_nb1=N_KV * 2 - 2)),
    ("k_nb1_short", REFUSED, dict(k_nb1=ROW_Q80 - 2)),
    ("v_nb1_short", REFUSED, dict(v_nb1=ROW_Q80 - 2)),
    ("q4_0_k_nb1_short", REFUSED, dict(Q40_PAIR, k_nb1=ROW_Q40 - 2)),
    ("q4_0_v_nb1_short", REFUSED, dict(Q40_PAIR, v_nb1=ROW_Q40 - 2)),
    ("d64_k_nb1_66", REFUSED, dict(D=64, k_nb1=66)),  # two blocks of 34 at D 64
    ("q_nb1_short", REFUSED, dict(q_nb1=D * 4 - 16)),
    ("dst_nb1_short", REFUSED, dict(dst_nb1=D * 4 - 16)),
    ("flags_1", REFUSED, dict(flags=1)),
    # step 5
    ("workspace_one_byte_short", REFUSED, FAQ_SHORT_WS),
    # two consecutive steps violated: the earlier one answers
    ("steps_1_2_negative_D_and_n_q_0", REFUSED, dict(D=-128, n_q=0)),
    ("steps_2_3_ne3_0_and_f16_pair", EMPTY, dict(F16_PAIR, ne3=0)),
    ("steps_3_4_d96_and_null_Q", REFUSED, dict(D=96, Q=None)),
    ("steps_4_5_flags_1_and_short_workspace", REFUSED, dict(FAQ_SHORT_WS, flags=1)),
    # two clauses of one step: the documented order inside it
    ("step_3_f16_pair_before_d96", REFUSED, dict(F16_PAIR, D=96)),
    ("step_3_pair_before_d96", REFUSED, dict(Vtype=T.Q4_0, D=96)),
    ("step_3_d96_before_max_bias", REFUSED, dict(D=96, max_bias=1.0)),
    ("step_3_max_bias_before_slices", REFUSED, dict(max_bias=1.0, n_head=256, ne3=256)),
    ("step_3_slices_before_n_kv_0", REFUSED, dict(n_head=256, ne3=256, n_kv=0)),
    ("step_4_null_before_n_head_kv", REFUSED, dict(V=None, n_head_kv=3)),
    ("step_4_n_head_kv_before_alignment", REFUSED, dict(n_head_kv=3, q_nb2=D * 4 + 8)),
    ("step_4_q_dst_alignment_before_k_v_alignment", REFUSED, dict(dst_nb3=N_Q * HEADS * D * 4 + 8, K=K_AT + 1)),
    ("step_4_k_v_alignment_before_mask", REFUSED, dict(K=K_AT + 1, mask=MASK_AT + 1)),
    ("step_4_mask_before_row_strides", REFUSED, dict(mask_nb1=N_KV * 2 - 2, k_nb1=ROW_Q80 - 2)),
    ("step_4_row_strides_before_flags", REFUSED, dict(k_nb1=ROW_Q80 - 2, flags=1)),
]

FAQ_UNPLACED = [
    ("every_pointer_null", NO_POINTERS, None),
    ("k_pointer_8", dict(NO_POINTERS, K=8), None),  # (lfamd_flash_attn refuses it: its K rows are loaded 16 bytes at a time)
    ("k_pointer_1", dict(NO_POINTERS, K=1), "k_base_plus_1"),
    ("q_pointer_8", dict(NO_POINTERS, Q=8), "q_base_plus_8"),
    ("workspace_one_byte_short", FAQ_SHORT_WS, None),
    ("null_workspace_with_a_size", dict(ws=None, ws_bytes=16), None),
    ("f16_pair", dict(NO_POINTERS, **F16_PAIR), "f16_pair"),
    ("d96", dict(NO_POINTERS, D=96), "d96"),
    ("k_nb1_short", dict(NO_POINTERS, k_nb1=ROW_Q80 - 2), "k_nb1_short"),
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

# ---- lfamd_mul_mat_batched and lfamd_mul_mat_batched_q: one argument list, one table (csrc/mul_mat_batched_common.h), the type, the
# k limits and A's row taken from the entry point's descriptor.  The control: the KQ product of the flash-attention control's operands —
# A the permuted K cache view (6 rows of k = 128 per KV head), B the query [n][heads][k], C contiguous [m, n, heads].  Neither call
# has a check function: the refused and the empty cases go to the entry point, where no GPU is present, and nowhere else.
M, K, N = N_KV, D, N_Q
MMB_ARGS = ("Atype", "A", "m", "k", "a_nb1", "a_nb2", "a_nb3", "a_ne2", "a_ne3", "B", "n", "b_nb1", "b_nb2", "b_nb3", "ne2", "ne3", "C", "c_nb1",
            "c_nb2", "c_nb3", "flags", "stream")
A_AT, B_AT, C_AT = K_AT, Q_AT, DST_AT


def _mmb_control(atype, row):
    return dict(Atype=atype, A=A_AT, m=M, k=K, a_nb1=KVH * row, a_nb2=row, a_nb3=M * KVH * row, a_ne2=KVH, a_ne3=1, B=B_AT, n=N,
                b_nb1=HEADS * K * 4, b_nb2=K * 4, b_nb3=N * HEADS * K * 4, ne2=HEADS, ne3=1, C=C_AT, c_nb1=M * 4, c_nb2=N * M * 4,
                c_nb3=HEADS * N * M * 4, flags=0, stream=None)


MMB_CONTROL = _mmb_control(T.F16, K * 2)
MMQ_CONTROL = _mmb_control(T.Q8_0, ROW_Q80)
MMB_NO_POINTERS = dict(A=None, B=None, C=None)


def _mmb_cases(row, other_type):
    """The rows the two calls answer alike; `row`: the control's A row in bytes, `other_type`: a type the call does not serve."""
    return [
        ("control", PASSES, {}),
        # step 1
        ("negative_m", REFUSED, dict(m=-1)),
        ("negative_k", REFUSED, dict(k=-32)),
        ("negative_n", REFUSED, dict(n=-1)),
        ("negative_ne2", REFUSED, dict(ne2=-8)),
        ("negative_ne3", REFUSED, dict(ne3=-1)),
        ("negative_a_ne2", REFUSED, dict(a_ne2=-2)),
        ("negative_a_ne3", REFUSED, dict(a_ne3=-1)),
        # step 2: no pointer, type, stride or flag is looked at
        ("m_0", EMPTY, dict(MMB_NO_POINTERS, m=0, Atype=other_type)),
        ("n_0", EMPTY, dict(MMB_NO_POINTERS, n=0, flags=1)),
        ("ne2_0", EMPTY, dict(MMB_NO_POINTERS, ne2=0, a_nb1=1)),
        ("ne3_0", EMPTY, dict(MMB_NO_POINTERS, ne3=0, a_ne3=0)),
        # step 3
        ("other_type", REFUSED, dict(Atype=other_type)),
        ("type_q6_k", REFUSED, dict(Atype=T.Q6_K)),
        ("ne2_65536", REFUSED, dict(ne2=65536)),
        ("ne3_65536", REFUSED, dict(ne3=65536)),
        ("ne2_256_ne3_256", REFUSED, dict(ne2=256, ne3=256)),
        ("n_column_tiles", REFUSED, dict(n=64 * 65535 + 1)),
        ("m_2_32_plus_1", REFUSED, dict(m=(1 << 32) + 1)),
        # step 4, clause by clause
        ("null_A", REFUSED, dict(A=None)),
        ("null_B", REFUSED, dict(B=None)),
        ("null_C", REFUSED, dict(C=None)),
        ("a_ne2_0", REFUSED, dict(a_ne2=0)),
        ("a_ne3_0", REFUSED, dict(a_ne3=0)),
        ("a_ne2_3", REFUSED, dict(a_ne2=3)),
        ("ne3_3_a_ne3_2", REFUSED, dict(ne3=3, a_ne3=2)),
        ("a_nb1_short", REFUSED, dict(a_nb1=row - 2)),
        ("b_nb1_short", REFUSED, dict(b_nb1=K * 4 - 4)),
        ("c_nb1_short", REFUSED, dict(c_nb1=M * 4 - 4)),
        ("a_base_plus_1", REFUSED, dict(A=A_AT + 1)),
        ("a_nb2_plus_1", REFUSED, dict(a_nb2=row + 1)),
        ("a_nb3_plus_1", REFUSED, dict(a_nb3=M * KVH * row + 1)),
        ("b_base_plus_2", REFUSED, dict(B=B_AT + 2)),
        ("b_nb2_plus_2", REFUSED, dict(b_nb2=K * 4 + 2)),
        ("c_base_plus_2", REFUSED, dict(C=C_AT + 2)),
        ("c_nb3_plus_2", REFUSED, dict(c_nb3=HEADS * N * M * 4 + 2)),
        ("flags_1", REFUSED, dict(flags=1)),
        # what the control may do and still reach the last row: A on a 2-byte boundary and no better, A's slices in front of its rows
        ("a_base_plus_2_reaches_flags", REFUSED, dict(A=A_AT + 2, flags=1)),
        ("k_0_reaches_flags", REFUSED, dict(k=0, flags=1)),
        # two consecutive steps violated: the earlier one answers
        ("steps_1_2_negative_k_and_m_0", REFUSED, dict(k=-32, m=0)),
        ("steps_2_3_n_0_and_other_type", EMPTY, dict(n=0, Atype=other_type)),
        ("steps_3_4_other_type_and_null_A", REFUSED, dict(Atype=other_type, A=None)),
        ("steps_3_4_slices_and_null_B", REFUSED, dict(ne2=256, ne3=256, B=None)),
        # two clauses of one step: the documented order inside it
        ("step_3_type_before_slices", REFUSED, dict(Atype=other_type, ne2=65536)),
        ("step_4_null_before_groups", REFUSED, dict(C=None, a_ne2=3)),
        ("step_4_groups_before_row_strides", REFUSED, dict(a_ne2=3, b_nb1=K * 4 - 4)),
        ("step_4_row_strides_before_a_alignment", REFUSED, dict(c_nb1=M * 4 - 4, A=A_AT + 1)),
        ("step_4_a_alignment_before_b_c_alignment", REFUSED, dict(a_nb2=row + 1, B=B_AT + 2)),
        ("step_4_b_c_alignment_before_flags", REFUSED, dict(C=C_AT + 2, flags=1)),
    ]


# the F16 call's descriptor has no k limit and k_mult 1: a long or ragged k reaches the last row
MMB_CASES = _mmb_cases(K * 2, T.Q8_0) + [
    ("type_f32", REFUSED, dict(Atype=T.F32)),
    ("k_2048_reaches_flags", REFUSED, dict(k=2048, a_nb1=KVH * 4096, a_nb2=4096, a_nb3=M * KVH * 4096, b_nb1=HEADS * 8192, b_nb2=8192,
                                           b_nb3=HEADS * 8192, flags=1)),
    ("k_100_reaches_flags", REFUSED, dict(k=100, flags=1)),
    # A's row is 2 k bytes: the control's a_nb1 of 512 holds k = 256 and not k = 257
    ("k_256_reaches_flags", REFUSED, dict(k=256, b_nb1=HEADS * 1040, b_nb2=1040, b_nb3=HEADS * 1040, flags=1)),
    ("k_257_a_row_short", REFUSED, dict(k=257, b_nb1=HEADS * 1040, b_nb2=1040, b_nb3=HEADS * 1040)),
]
ROW_K1056 = 1056 // 32 * 34
MMQ_CASES = _mmb_cases(ROW_Q80, T.F16) + [
    ("control_q4_0", PASSES, dict(Atype=T.Q4_0, a_nb1=KVH * ROW_Q40, a_nb2=ROW_Q40, a_nb3=M * KVH * ROW_Q40)),
    ("type_q8_0_pad256", REFUSED, dict(Atype=T.Q8_0 | _hip.TYPE_PAD256)),
    ("type_q8_1", REFUSED, dict(Atype=T.Q8_1)),
    ("type_bf16", REFUSED, dict(Atype=T.BF16)),
    ("k_1056", REFUSED, dict(k=1056, a_nb1=KVH * ROW_K1056, a_nb2=ROW_K1056, a_nb3=M * KVH * ROW_K1056, b_nb1=HEADS * 1056 * 4, b_nb2=1056 * 4,
                             b_nb3=HEADS * 1056 * 4)),
    ("k_1024_reaches_flags", REFUSED, dict(k=1024, a_nb1=KVH * 1088, a_nb2=1088, a_nb3=M * KVH * 1088, b_nb1=HEADS * 4096, b_nb2=4096,
                                           b_nb3=HEADS * 4096, flags=1)),
    ("k_48", REFUSED, dict(k=48)),
    ("k_1", REFUSED, dict(k=1)),
    # A's row is the type's: 4 blocks of 18 (Q4_0), 20 (Q4_1), 22 (Q5_0), 24 (Q5_1), 18 (IQ4_NL) bytes
    ("q4_0_row_72_reaches_flags", REFUSED, dict(Atype=T.Q4_0, a_nb1=72, flags=1)),
    ("q4_0_row_70", REFUSED, dict(Atype=T.Q4_0, a_nb1=70)),
    ("q4_1_row_80_reaches_flags", REFUSED, dict(Atype=T.Q4_1, a_nb1=80, flags=1)),
    ("q4_1_row_78", REFUSED, dict(Atype=T.Q4_1, a_nb1=78)),
    ("q5_0_row_88_reaches_flags", REFUSED, dict(Atype=T.Q5_0, a_nb1=88, flags=1)),
    ("q5_0_row_86", REFUSED, dict(Atype=T.Q5_0, a_nb1=86)),
    ("q5_1_row_96_reaches_flags", REFUSED, dict(Atype=T.Q5_1, a_nb1=96, flags=1)),
    ("q5_1_row_94", REFUSED, dict(Atype=T.Q5_1, a_nb1=94)),
    ("iq4_nl_row_72_reaches_flags", REFUSED, dict(Atype=T.IQ4_NL, a_nb1=72, flags=1)),
    ("iq4_nl_row_70", REFUSED, dict(Atype=T.IQ4_NL, a_nb1=70)),
    # the descriptor's rows among the others, in the documented order
    ("step_3_type_before_k_1056", REFUSED, dict(Atype=T.F16, k=1056)),
    ("step_3_k_1056_before_slices", REFUSED, dict(k=1056, ne2=65536)),
    ("steps_3_4_k_1056_and_null_A", REFUSED, dict(k=1056, A=None)),
    ("step_4_groups_before_k_48", REFUSED, dict(a_ne2=3, k=48)),
    ("step_4_k_48_before_row_strides", REFUSED, dict(k=48, a_nb1=2)),
]

OPERATORS = {"lfamd_flash_attn": (FA_ARGS, FA_CONTROL, FA_CASES, FA_UNPLACED), "lfamd_cpy": (CPY_ARGS, CPY_CONTROL, CPY_CASES, CPY_UNPLACED),
             "lfamd_flash_attn_q": (FA_ARGS, FAQ_CONTROL, FAQ_CASES, FAQ_UNPLACED),
             "lfamd_mul_mat_batched": (MMB_ARGS, MMB_CONTROL, MMB_CASES, []), "lfamd_mul_mat_batched_q": (MMB_ARGS, MMQ_CONTROL, MMQ_CASES, [])}
# what the check functions' argument lists leave out; an operator that is not here has no check function
NOT_IN_CHECK = {"lfamd_flash_attn": ("scale", "stream"), "lfamd_flash_attn_q": ("scale", "stream"), "lfamd_cpy": ("stream",)}

_vp, _sz, _l, _i, _u, _f = C.c_void_p, C.c_size_t, C.c_long, C.c_int, C.c_uint, C.c_float
_FA_TYPES = dict(Q=_vp, K=_vp, V=_vp, mask=_vp, dst=_vp, ws=_vp, stream=_vp, Ktype=_i, Vtype=_i, scale=_f, max_bias=_f, flags=_u,
                 D=_l, n_q=_l, n_kv=_l, n_head=_l, n_head_kv=_l, ne3=_l)
_CPY_TYPES = dict(src_type=_i, dst_type=_i, src=_vp, dst=_vp, stream=_vp, flags=_u, src_ne=C.POINTER(_l), dst_ne=C.POINTER(_l),
                  src_nb=C.POINTER(_sz), dst_nb=C.POINTER(_sz))
_MMB_TYPES = dict(Atype=_i, A=_vp, B=_vp, C=_vp, stream=_vp, flags=_u, m=_l, k=_l, n=_l, a_ne2=_l, a_ne3=_l, ne2=_l, ne3=_l)
_TYPES = {"lfamd_flash_attn": _FA_TYPES, "lfamd_flash_attn_q": _FA_TYPES, "lfamd_cpy": _CPY_TYPES, "lfamd_mul_mat_batched": _MMB_TYPES,
          "lfamd_mul_mat_batched_q": _MMB_TYPES}


def _ctype(op, name):
    return _TYPES[op].get(name, _sz)


def bind(path):
    """The library at `path` with the entry points' signatures, and the check functions' where it has them."""
    import torch  # noqa: F401  (first: its HIP runtime is the one the library must resolve to, as in llamafile_amd/_hip.py)
    lib = C.CDLL(path)
    lib.lfamd_last_error.restype = C.c_char_p
    for op, (names, _, _, _) in OPERATORS.items():
        getattr(lib, op).argtypes = [_ctype(op, n) for n in names]
        if op in NOT_IN_CHECK and hasattr(lib, op + "_check"):
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
