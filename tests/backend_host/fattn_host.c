/*
 * fattn_host.c — TEST INFRASTRUCTURE: backend_host.c's host side for GGML_OP_FLASH_ATTN_EXT.  Its operator table names
 * FLASH_ATTN_EXT at a number that is not upstream's (the module must find it by name), or — FATTN_HOST_NO_NAME=1 — not at all,
 * the way a ggml build from before the operator does: the module then links and is never offered the node.
 *
 *   fattn_host <module.so> decline <case>   what supports_op says for one node ("accepted" / "declined"); nothing is computed.
 *       control (F16 K / V, D = 128, F16 mask), control_nomask, d96, max_bias, prec_f32, q4_0_k, view_offs (Q a view 8 bytes into
 *       its parent, no address yet), control_view_offs16; and, each the control node with one change: q_f16, v_f32, dst_f16, q_nb0,
 *       dst_strided, v_ne1, v_ne2, k_ne3, heads_3kv (8 heads on 3 KV heads), dst_ne1, mask_f32, mask_ne0, mask_ne1, mask_ne2,
 *       mask_nb1_odd, k_nb1_8 (not a multiple of 16), slices (n_head * ne3 = 65536), q_nb1_short and k_nb1_short (rows 256 / 128 bytes
 *       apart: multiples of 16, half a row of D = 128)
 *   fattn_host <module.so> run <Q.bin> <K.bin> <V.bin> <mask.bin> <out.bin> [<n_q> <n_kv> <mask rows> [<Q.bin> ... <mask rows>]]
 *       one graph_compute of one grouped-query node per group of arguments, in their order: 2 KV heads x 4, D = 128, n_q = 17,
 *       n_kv = 65 and a mask of 32 rows where the three numbers are not given; Q memory [n_q][n_head][D], K / V the permuted cache
 *       views (memory [n_kv][kv head][D]), the mask F16 [n_kv x mask rows] (padded beyond n_q), dst contiguous [D, n_head, n_q];
 *       op_params = {1 / sqrt(128), 0, GGML_PREC_DEFAULT}
 */
#include <math.h>

#define main backend_host_main
#include "backend_host.c"
#undef main

#define OP_FLASH_ATTN_EXT 47 /* (upstream's number differs) */

static GGML_CALL const char *h_op_name_fa(int op) {
    if (op == OP_FLASH_ATTN_EXT && !getenv("FATTN_HOST_NO_NAME"))
        return "FLASH_ATTN_EXT";
    return op >= 0 && op < 60 ? h_op_name(op) : NULL; /* a table of 60 names */
}

enum { D = 128, N_Q = 17, N_KV = 65, KVH = 2, HEADS = 8, MASK_ROWS = 32, MAX_NODES = 4 };

static void fa_node(struct ggml_tensor *Q, struct ggml_tensor *K, struct ggml_tensor *V, struct ggml_tensor *M, struct ggml_tensor *OUT, long d,
                    int ktype, long n_q, long n_kv, long mask_rows) {
    shape(Q, LFAMD_TYPE_F32, d, n_q, HEADS, 1); /* memory [n_q][heads][d] */
    Q->nb[1] = (size_t)HEADS * d * 4, Q->nb[2] = (size_t)d * 4, Q->nb[3] = (size_t)n_q * HEADS * d * 4;
    shape(K, ktype, d, n_kv, KVH, 1); /* memory [n_kv][kv heads][row] */
    const size_t row = K->nb[1];
    K->nb[1] = KVH * row, K->nb[2] = row, K->nb[3] = (size_t)n_kv * KVH * row;
    shape(V, LFAMD_TYPE_F16, d, n_kv, KVH, 1);
    V->nb[1] = (size_t)KVH * d * 2, V->nb[2] = (size_t)d * 2, V->nb[3] = (size_t)n_kv * KVH * d * 2;
    shape(M, LFAMD_TYPE_F16, n_kv, mask_rows, 1, 1);
    shape(OUT, LFAMD_TYPE_F32, d, HEADS, n_q, 1);
    const float scale = 1.0f / sqrtf((float)d), max_bias = 0.0f;
    memcpy(&OUT->op_params[0], &scale, 4);
    memcpy(&OUT->op_params[1], &max_bias, 4);
    OUT->op_params[2] = 0; /* GGML_PREC_DEFAULT */
    OUT->op = OP_FLASH_ATTN_EXT, OUT->src[0] = Q, OUT->src[1] = K, OUT->src[2] = V, OUT->src[3] = M;
}

static int fa_decline(ggml_backend_t be, ggml_backend_buffer_type_t buft, const char *what) {
    const size_t align = buft->iface.get_alignment(buft);
    ggml_backend_buffer_t buf = buft->iface.alloc_buffer(buft, 1 << 21);
    if (!buf) return 10;
    struct ggml_tensor Q, K, V, M, OUT;
    fa_node(&Q, &K, &V, &M, &OUT, !strcmp(what, "d96") ? 96 : D, !strcmp(what, "q4_0_k") ? LFAMD_TYPE_Q4_0 : LFAMD_TYPE_F16, N_Q, N_KV, MASK_ROWS);
    size_t off = align;
    place(&Q, buf, &off, align);
    off += align;
    place(&K, buf, &off, align);
    place(&V, buf, &off, align);
    place(&M, buf, &off, align);
    place(&OUT, buf, &off, align);
    if (!strcmp(what, "control") || !strcmp(what, "d96") || !strcmp(what, "q4_0_k")) {
        /* (the node as built) */
    } else if (!strcmp(what, "control_nomask")) {
        OUT.src[3] = NULL;
    } else if (!strcmp(what, "max_bias")) {
        const float b = 8.0f;
        memcpy(&OUT.op_params[1], &b, 4);
    } else if (!strcmp(what, "prec_f32")) {
        OUT.op_params[2] = 1; /* GGML_PREC_F32 */
    } else if (!strcmp(what, "view_offs") || !strcmp(what, "control_view_offs16")) {
        Q.view_src = &OUT, Q.view_offs = !strcmp(what, "view_offs") ? 8 : 16, Q.data = NULL;
    } else if (!strcmp(what, "q_f16")) { /* from here on: the control node with ONE field changed (nothing is computed) */
        Q.type = LFAMD_TYPE_F16;
    } else if (!strcmp(what, "v_f32")) {
        V.type = LFAMD_TYPE_F32;
    } else if (!strcmp(what, "dst_f16")) {
        OUT.type = LFAMD_TYPE_F16;
    } else if (!strcmp(what, "q_nb0")) {
        Q.nb[0] = 8;
    } else if (!strcmp(what, "dst_strided")) {
        OUT.nb[1] += 16, OUT.nb[2] = OUT.nb[1] * HEADS, OUT.nb[3] = OUT.nb[2] * N_Q; /* rows 16 bytes apart: aligned, not contiguous */
    } else if (!strcmp(what, "v_ne1")) {
        V.ne[1] = N_KV + 1;
    } else if (!strcmp(what, "v_ne2")) {
        V.ne[2] = 1;
    } else if (!strcmp(what, "k_ne3")) {
        K.ne[3] = 2;
    } else if (!strcmp(what, "heads_3kv")) {
        K.ne[2] = V.ne[2] = 3;
    } else if (!strcmp(what, "dst_ne1")) {
        OUT.ne[1] = HEADS + 1, OUT.nb[2] = OUT.nb[1] * OUT.ne[1], OUT.nb[3] = OUT.nb[2] * N_Q; /* (still contiguous) */
    } else if (!strcmp(what, "mask_f32")) {
        M.type = LFAMD_TYPE_F32;
    } else if (!strcmp(what, "mask_ne0")) {
        M.ne[0] = N_KV - 1;
    } else if (!strcmp(what, "mask_ne1")) {
        M.ne[1] = N_Q - 1;
    } else if (!strcmp(what, "mask_ne2")) {
        M.ne[2] = 2;
    } else if (!strcmp(what, "mask_nb1_odd")) {
        M.nb[1] = 2 * N_KV + 1;
    } else if (!strcmp(what, "k_nb1_8")) {
        K.nb[1] += 8;
    } else if (!strcmp(what, "q_nb1_short")) {
        Q.nb[1] = 256; /* a row of 128 floats is 512 bytes */
    } else if (!strcmp(what, "k_nb1_short")) {
        K.nb[1] = 128; /* a row of 128 halves is 256 bytes */
    } else if (!strcmp(what, "slices")) {
        Q.ne[3] = K.ne[3] = V.ne[3] = OUT.ne[3] = 8192; /* 8 heads x 8192 = 65536 */
    } else {
        fprintf(stderr, "unknown case %s\n", what);
        return 2;
    }
    printf("%s\n", be->iface.supports_op(be, &OUT) ? "accepted" : "declined");
    buf->iface.free_buffer(buf);
    be->iface.free(be);
    return 0;
}

/* argv[3 ..]: per node <Q> <K> <V> <mask> <out> <n_q> <n_kv> <mask rows>; the three numbers of the first node may be left out */
static int fa_run(ggml_backend_t be, ggml_backend_buffer_type_t buft, int argc, char **argv) {
    const int n_nodes = argc <= 8 ? 1 : (argc - 3) / 8;
    if (n_nodes > MAX_NODES || (argc > 8 && (argc - 3) % 8 != 0)) { fprintf(stderr, "usage\n"); return 2; }
    struct ggml_tensor Q[MAX_NODES], K[MAX_NODES], V[MAX_NODES], M[MAX_NODES], OUT[MAX_NODES];
    struct ggml_tensor *nodes[MAX_NODES];
    void *hq[MAX_NODES], *hk[MAX_NODES], *hv[MAX_NODES], *hm[MAX_NODES];
    size_t nq[MAX_NODES], nk[MAX_NODES], nv[MAX_NODES], nm[MAX_NODES], kv_bytes = 0, c_bytes = 0;
    const size_t align = buft->iface.get_alignment(buft);
    for (int i = 0; i < n_nodes; i++) {
        char **a = argv + 3 + 8 * i;
        const bool dims = argc > 8;
        hq[i] = slurp(a[0], &nq[i]), hk[i] = slurp(a[1], &nk[i]), hv[i] = slurp(a[2], &nv[i]), hm[i] = slurp(a[3], &nm[i]);
        fa_node(&Q[i], &K[i], &V[i], &M[i], &OUT[i], D, LFAMD_TYPE_F16, dims ? atol(a[5]) : N_Q, dims ? atol(a[6]) : N_KV, dims ? atol(a[7]) : MASK_ROWS);
        if (h_nbytes(&Q[i]) != nq[i] || h_nbytes(&K[i]) != nk[i] || h_nbytes(&V[i]) != nv[i] || h_nbytes(&M[i]) != nm[i]) {
            fprintf(stderr, "input size mismatch (node %d)\n", i);
            return 9;
        }
        kv_bytes += nk[i] + nv[i] + 2 * align, c_bytes += nq[i] + nm[i] + h_nbytes(&OUT[i]) + 3 * align;
        nodes[i] = &OUT[i];
    }
    ggml_backend_buffer_t kvbuf = buft->iface.alloc_buffer(buft, kv_bytes + 8 * align);
    ggml_backend_buffer_t cbuf = buft->iface.alloc_buffer(buft, c_bytes + 8 * align);
    if (!kvbuf || !cbuf) return 10;
    size_t ko = 2 * align, co = align; /* every operand at a non-zero offset */
    for (int i = 0; i < n_nodes; i++) {
        place(&K[i], kvbuf, &ko, align);
        place(&V[i], kvbuf, &ko, align);
        place(&Q[i], cbuf, &co, align);
        place(&M[i], cbuf, &co, align);
        place(&OUT[i], cbuf, &co, align);
        kvbuf->iface.set_tensor(kvbuf, &K[i], hk[i], 0, nk[i]);
        kvbuf->iface.set_tensor(kvbuf, &V[i], hv[i], 0, nv[i]);
        cbuf->iface.set_tensor(cbuf, &Q[i], hq[i], 0, nq[i]);
        cbuf->iface.set_tensor(cbuf, &M[i], hm[i], 0, nm[i]);
        if (!be->iface.supports_op(be, &OUT[i])) { fprintf(stderr, "supports_op says no (node %d)\n", i); return 11; }
    }
    struct ggml_cgraph g = {n_nodes, n_nodes, 0, nodes, NULL, NULL};
    if (be->iface.graph_compute(be, &g) != GGML_STATUS_SUCCESS) { fprintf(stderr, "graph_compute failed\n"); return 12; }
    be->iface.synchronize(be);
    for (int i = 0; i < n_nodes; i++) {
        const size_t no = h_nbytes(&OUT[i]);
        void *ho = malloc(no);
        cbuf->iface.get_tensor(cbuf, &OUT[i], ho, 0, no);
        dump(argv[3 + 8 * i + 4], "", ho, no);
        free(ho);
    }
    cbuf->iface.free_buffer(cbuf);
    kvbuf->iface.free_buffer(kvbuf);
    be->iface.free(be);
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    api.ggml_op_name = h_op_name_fa;
    void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 3; }
    bool GGML_CALL (*link)(const struct ggml_backend_api *) = dlsym(lib, "ggml_cuda_link");
    ggml_backend_buffer_type_t GGML_CALL (*buffer_type)(int) = dlsym(lib, "ggml_backend_cuda_buffer_type");
    ggml_backend_t GGML_CALL (*backend_init)(int) = dlsym(lib, "ggml_backend_cuda_init");
    if (!link || !buffer_type || !backend_init) { fprintf(stderr, "missing symbol\n"); return 4; }
    if (!link(&api)) { fprintf(stderr, "link failed\n"); return 5; }
    ggml_backend_buffer_type_t buft = buffer_type(0);
    ggml_backend_t be = backend_init(0);
    if (!buft || !be) return 8;
    if (!strcmp(argv[2], "decline"))
        return argc < 4 ? 2 : fa_decline(be, buft, argv[3]);
    if (!strcmp(argv[2], "run"))
        return argc < 8 ? 2 : fa_run(be, buft, argc, argv);
    fprintf(stderr, "unknown mode %s\n", argv[2]);
    return 2;
}
