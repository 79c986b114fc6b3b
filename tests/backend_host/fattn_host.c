/*
 * fattn_host.c — TEST INFRASTRUCTURE: backend_host.c's host side for GGML_OP_FLASH_ATTN_EXT.  Its operator table names
 * FLASH_ATTN_EXT at a number that is not upstream's (the module must find it by name), or — FATTN_HOST_NO_NAME=1 — not at all,
 * the way a ggml build from before the operator does: the module then links and is never offered the node.
 *
 *   fattn_host <module.so> decline <case>   what supports_op says for one node ("accepted" / "declined"); nothing is computed.
 *       control (F16 K / V, D = 128, F16 mask), control_nomask, d96, max_bias, prec_f32, q4_0_k, view_offs (Q a view 8 bytes into
 *       its parent, no address yet), control_view_offs16
 *   fattn_host <module.so> run <Q.bin> <K.bin> <V.bin> <mask.bin> <out.bin>
 *       one graph_compute of a grouped-query node: 2 KV heads x 4, n_q = 17, n_kv = 65, D = 128; Q memory [n_q][n_head][D], K / V
 *       the permuted cache views (memory [n_kv][kv head][D]), the mask F16 [65 x 32] (padded to 32 rows), dst contiguous
 *       [D, n_head, n_q]; op_params = {1 / sqrt(128), 0, GGML_PREC_DEFAULT}
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

enum { D = 128, N_Q = 17, N_KV = 65, KVH = 2, HEADS = 8, MASK_ROWS = 32 };

static void fa_node(struct ggml_tensor *Q, struct ggml_tensor *K, struct ggml_tensor *V, struct ggml_tensor *M, struct ggml_tensor *OUT, long d,
                    int ktype) {
    shape(Q, LFAMD_TYPE_F32, d, N_Q, HEADS, 1); /* memory [n_q][heads][d] */
    Q->nb[1] = (size_t)HEADS * d * 4, Q->nb[2] = (size_t)d * 4, Q->nb[3] = (size_t)N_Q * HEADS * d * 4;
    shape(K, ktype, d, N_KV, KVH, 1); /* memory [n_kv][kv heads][row] */
    const size_t row = K->nb[1];
    K->nb[1] = KVH * row, K->nb[2] = row, K->nb[3] = (size_t)N_KV * KVH * row;
    shape(V, LFAMD_TYPE_F16, d, N_KV, KVH, 1);
    V->nb[1] = (size_t)KVH * d * 2, V->nb[2] = (size_t)d * 2, V->nb[3] = (size_t)N_KV * KVH * d * 2;
    shape(M, LFAMD_TYPE_F16, N_KV, MASK_ROWS, 1, 1);
    shape(OUT, LFAMD_TYPE_F32, d, HEADS, N_Q, 1);
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
    fa_node(&Q, &K, &V, &M, &OUT, !strcmp(what, "d96") ? 96 : D, !strcmp(what, "q4_0_k") ? LFAMD_TYPE_Q4_0 : LFAMD_TYPE_F16);
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
    } else {
        fprintf(stderr, "unknown case %s\n", what);
        return 2;
    }
    printf("%s\n", be->iface.supports_op(be, &OUT) ? "accepted" : "declined");
    buf->iface.free_buffer(buf);
    be->iface.free(be);
    return 0;
}

static int fa_run(ggml_backend_t be, ggml_backend_buffer_type_t buft, char **argv) {
    size_t nq, nk, nv, nm;
    void *hq = slurp(argv[3], &nq), *hk = slurp(argv[4], &nk), *hv = slurp(argv[5], &nv), *hm = slurp(argv[6], &nm);
    struct ggml_tensor Q, K, V, M, OUT;
    fa_node(&Q, &K, &V, &M, &OUT, D, LFAMD_TYPE_F16);
    if (h_nbytes(&Q) != nq || h_nbytes(&K) != nk || h_nbytes(&V) != nv || h_nbytes(&M) != nm) { fprintf(stderr, "input size mismatch\n"); return 9; }
    const size_t align = buft->iface.get_alignment(buft);
    ggml_backend_buffer_t kvbuf = buft->iface.alloc_buffer(buft, nk + nv + 8 * align);
    ggml_backend_buffer_t cbuf = buft->iface.alloc_buffer(buft, nq + nm + h_nbytes(&OUT) + 8 * align);
    if (!kvbuf || !cbuf) return 10;
    size_t ko = 2 * align, co = align; /* every operand at a non-zero offset */
    place(&K, kvbuf, &ko, align);
    place(&V, kvbuf, &ko, align);
    place(&Q, cbuf, &co, align);
    place(&M, cbuf, &co, align);
    place(&OUT, cbuf, &co, align);
    kvbuf->iface.set_tensor(kvbuf, &K, hk, 0, nk);
    kvbuf->iface.set_tensor(kvbuf, &V, hv, 0, nv);
    cbuf->iface.set_tensor(cbuf, &Q, hq, 0, nq);
    cbuf->iface.set_tensor(cbuf, &M, hm, 0, nm);
    if (!be->iface.supports_op(be, &OUT)) { fprintf(stderr, "supports_op says no\n"); return 11; }
    struct ggml_tensor *nodes[1] = {&OUT};
    struct ggml_cgraph g = {1, 1, 0, nodes, NULL, NULL};
    if (be->iface.graph_compute(be, &g) != GGML_STATUS_SUCCESS) { fprintf(stderr, "graph_compute failed\n"); return 12; }
    be->iface.synchronize(be);
    const size_t no = h_nbytes(&OUT);
    void *ho = malloc(no);
    cbuf->iface.get_tensor(cbuf, &OUT, ho, 0, no);
    dump(argv[7], "", ho, no);
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
        return argc < 8 ? 2 : fa_run(be, buft, argv);
    fprintf(stderr, "unknown mode %s\n", argv[2]);
    return 2;
}
