/*
 * fattn_q_host.c — TEST INFRASTRUCTURE: backend_host.c's host side for GGML_OP_FLASH_ATTN_EXT on a Q8_0 / Q4_0 K and V cache
 * (-fa -ctk q8_0 -ctv q8_0).  Its operator table names FLASH_ATTN_EXT and CPY at numbers that are not upstream's.
 *
 *   fattn_q_host <module.so> decline <case>   what supports_op says for one node ("accepted" / "declined"); nothing is computed.
 *       The node: 8 heads on 2 KV heads, D = 128, n_q = 17, n_kv = 65, F16 mask of 32 rows, K / V the permuted cache views.
 *       q8_0, q4_0 (the pair); q8_0_view2, q4_0_view2 (K a view 34 / 18 bytes into its parent, no address yet: a 2-byte boundary);
 *       q8_0_k_f16_v, f16_k_q8_0_v, q8_0_k_q4_0_v, q4_1 (a Q4_1 pair); and the q8_0 node with one change: d96, prec_f32, max_bias,
 *       v_ne1 (V one row longer), view_odd (K a view 35 bytes into its parent)
 *   fattn_q_host <module.so> store <k_cache> <v_cache> <k_cur> <v_cur> <Q> <mask> <out> <k_cache out> <v_cache out> <n_q>
 *       ONE graph_compute of three nodes on Q8_0 caches of 72 cells of 2 KV heads x 128 (the files hold their first contents, whole):
 *       CPY of k_cur (F32 [128, 2, 3]) into cells 62 .. 64 of K, CPY of v_cur (F32 [256, 3]) into cells 62 .. 64 of V, then
 *       FLASH_ATTN_EXT of 8 heads, n_q queries, over cells 0 .. 64 (mask F16 [65 x 32]); the result and both caches are read back
 *   fattn_q_host <module.so> run <type> <Q> <K> <V> <mask> <out> <n_q> <n_kv> <mask rows>
 *       one graph_compute of one node on K / V files of raw blocks (type: q8_0 / q4_0), memory [n_kv][kv head][row of blocks]
 */
#include <math.h>

#define main backend_host_main
#include "backend_host.c"
#undef main

#define OP_FLASH_ATTN_EXT 47 /* (upstream's numbers differ) */
#define OP_CPY 52

static GGML_CALL const char *h_op_name_faq(int op) {
    if (op == OP_CPY)
        return "CPY";
    if (op == OP_FLASH_ATTN_EXT)
        return "FLASH_ATTN_EXT";
    return op >= 0 && op < 60 ? h_op_name(op) : NULL; /* a table of 60 names */
}

enum { D = 128, N_Q = 17, N_KV = 65, KVH = 2, HEADS = 8, MASK_ROWS = 32, WIDTH = D * KVH, N_CTX = 72, HEAD = 62, N_TOK = 3 };

/* a cache view [d, n_kv, kv heads] of `type`, memory [n_kv][kv head][row] */
static void cache_view(struct ggml_tensor *t, int type, long d, long n_kv) {
    shape(t, type, d, n_kv, KVH, 1);
    const size_t row = t->nb[1];
    t->nb[1] = KVH * row, t->nb[2] = row, t->nb[3] = (size_t)n_kv * KVH * row;
}

static void fa_node(struct ggml_tensor *Q, struct ggml_tensor *K, struct ggml_tensor *V, struct ggml_tensor *M, struct ggml_tensor *OUT, long d,
                    int ktype, int vtype, long n_q, long n_kv, long mask_rows) {
    shape(Q, LFAMD_TYPE_F32, d, n_q, HEADS, 1); /* memory [n_q][heads][d] */
    Q->nb[1] = (size_t)HEADS * d * 4, Q->nb[2] = (size_t)d * 4, Q->nb[3] = (size_t)n_q * HEADS * d * 4;
    if (K)
        cache_view(K, ktype, d, n_kv);
    if (V)
        cache_view(V, vtype, d, n_kv);
    shape(M, LFAMD_TYPE_F16, n_kv, mask_rows, 1, 1);
    shape(OUT, LFAMD_TYPE_F32, d, HEADS, n_q, 1);
    const float scale = 1.0f / sqrtf((float)d), max_bias = 0.0f;
    memcpy(&OUT->op_params[0], &scale, 4);
    memcpy(&OUT->op_params[1], &max_bias, 4);
    OUT->op_params[2] = 0; /* GGML_PREC_DEFAULT */
    OUT->op = OP_FLASH_ATTN_EXT, OUT->src[0] = Q, OUT->src[1] = K, OUT->src[2] = V, OUT->src[3] = M;
}

static int type_of(const char *name) {
    return !strcmp(name, "q8_0") ? LFAMD_TYPE_Q8_0 : !strcmp(name, "q4_0") ? LFAMD_TYPE_Q4_0 : -1;
}

static int faq_decline(ggml_backend_t be, ggml_backend_buffer_type_t buft, const char *what) {
    const size_t align = buft->iface.get_alignment(buft);
    ggml_backend_buffer_t buf = buft->iface.alloc_buffer(buft, 1 << 21);
    if (!buf) return 10;
    int ktype = LFAMD_TYPE_Q8_0, vtype = LFAMD_TYPE_Q8_0;
    if (!strncmp(what, "q4_0", 4))
        ktype = vtype = LFAMD_TYPE_Q4_0;
    else if (!strcmp(what, "q8_0_k_f16_v"))
        vtype = LFAMD_TYPE_F16;
    else if (!strcmp(what, "f16_k_q8_0_v"))
        ktype = LFAMD_TYPE_F16;
    else if (!strcmp(what, "q8_0_k_q4_0_v"))
        vtype = LFAMD_TYPE_Q4_0;
    else if (!strcmp(what, "q4_1"))
        ktype = vtype = LFAMD_TYPE_Q4_1;
    struct ggml_tensor Q, K, V, M, OUT;
    fa_node(&Q, &K, &V, &M, &OUT, !strcmp(what, "d96") ? 96 : D, ktype, vtype, N_Q, N_KV, MASK_ROWS);
    size_t off = align;
    place(&Q, buf, &off, align);
    place(&K, buf, &off, align);
    place(&V, buf, &off, align);
    place(&M, buf, &off, align);
    place(&OUT, buf, &off, align);
    if (!strcmp(what, "q8_0") || !strcmp(what, "q4_0") || !strcmp(what, "q8_0_k_f16_v") || !strcmp(what, "f16_k_q8_0_v") ||
        !strcmp(what, "q8_0_k_q4_0_v") || !strcmp(what, "q4_1") || !strcmp(what, "d96")) {
        /* (the node as built) */
    } else if (!strcmp(what, "q8_0_view2") || !strcmp(what, "q4_0_view2")) {
        K.view_src = &V, K.view_offs = K.nb[0], K.data = NULL; /* one block in: 34 or 18 bytes */
    } else if (!strcmp(what, "view_odd")) {
        K.view_src = &V, K.view_offs = 35, K.data = NULL;
    } else if (!strcmp(what, "prec_f32")) {
        OUT.op_params[2] = 1; /* GGML_PREC_F32 */
    } else if (!strcmp(what, "max_bias")) {
        const float b = 8.0f;
        memcpy(&OUT.op_params[1], &b, 4);
    } else if (!strcmp(what, "v_ne1")) {
        V.ne[1] = N_KV + 1;
    } else {
        fprintf(stderr, "unknown case %s\n", what);
        return 2;
    }
    printf("%s\n", be->iface.supports_op(be, &OUT) ? "accepted" : "declined");
    buf->iface.free_buffer(buf);
    be->iface.free(be);
    return 0;
}

/* dst: a 1-D view of n elements, `offs` bytes into the cache tensor; node: the CPY of src into it (itself a view of dst) */
static void cpy_node(struct ggml_tensor *node, struct ggml_tensor *dst, struct ggml_tensor *src, struct ggml_tensor *cache, int64_t n, size_t offs) {
    shape(dst, cache->type, n, 1, 1, 1);
    dst->view_src = cache, dst->view_offs = offs, dst->buffer = cache->buffer, dst->data = (uint8_t *)cache->data + offs;
    *node = *dst;
    node->op = OP_CPY, node->src[0] = src, node->src[1] = dst;
}

static int faq_store(ggml_backend_t be, ggml_backend_buffer_type_t buft, char **argv) {
    const size_t align = buft->iface.get_alignment(buft);
    const long n_q = atol(argv[12]);
    size_t nkc, nvc, nk, nv, nq, nm;
    void *hkc = slurp(argv[3], &nkc), *hvc = slurp(argv[4], &nvc), *hk = slurp(argv[5], &nk), *hv = slurp(argv[6], &nv);
    void *hq = slurp(argv[7], &nq), *hm = slurp(argv[8], &nm);
    struct ggml_tensor KC, VC, KCUR, VCUR, KDST, VDST, KCPY, VCPY, Q, K, V, M, OUT;
    shape(&KC, LFAMD_TYPE_Q8_0, (int64_t)WIDTH * N_CTX, 1, 1, 1);
    shape(&VC, LFAMD_TYPE_Q8_0, (int64_t)WIDTH * N_CTX, 1, 1, 1);
    shape(&KCUR, LFAMD_TYPE_F32, D, KVH, N_TOK, 1);
    shape(&VCUR, LFAMD_TYPE_F32, WIDTH, N_TOK, 1, 1);
    fa_node(&Q, NULL, NULL, &M, &OUT, D, 0, 0, n_q, N_KV, MASK_ROWS);
    if (n_q < 1 || n_q > MASK_ROWS || h_nbytes(&KC) != nkc || h_nbytes(&VC) != nvc || h_nbytes(&KCUR) != nk || h_nbytes(&VCUR) != nv ||
        h_nbytes(&Q) != nq || h_nbytes(&M) != nm) {
        fprintf(stderr, "input size mismatch\n");
        return 9;
    }
    ggml_backend_buffer_t kvbuf = buft->iface.alloc_buffer(buft, nkc + nvc + 8 * align);
    ggml_backend_buffer_t cbuf = buft->iface.alloc_buffer(buft, nk + nv + nq + nm + h_nbytes(&OUT) + 16 * align);
    if (!kvbuf || !cbuf) return 10;
    size_t ko = 2 * align, co = align; /* every operand at a non-zero offset */
    place(&KC, kvbuf, &ko, align);
    place(&VC, kvbuf, &ko, align);
    place(&KCUR, cbuf, &co, align);
    place(&VCUR, cbuf, &co, align);
    place(&Q, cbuf, &co, align);
    place(&M, cbuf, &co, align);
    place(&OUT, cbuf, &co, align);
    kvbuf->iface.set_tensor(kvbuf, &KC, hkc, 0, nkc);
    kvbuf->iface.set_tensor(kvbuf, &VC, hvc, 0, nvc);
    cbuf->iface.set_tensor(cbuf, &KCUR, hk, 0, nk);
    cbuf->iface.set_tensor(cbuf, &VCUR, hv, 0, nv);
    cbuf->iface.set_tensor(cbuf, &Q, hq, 0, nq);
    cbuf->iface.set_tensor(cbuf, &M, hm, 0, nm);
    const size_t cell = nkc / N_CTX;
    cpy_node(&KCPY, &KDST, &KCUR, &KC, (int64_t)WIDTH * N_TOK, HEAD * cell);
    cpy_node(&VCPY, &VDST, &VCUR, &VC, (int64_t)WIDTH * N_TOK, HEAD * cell);
    /* the attention's views of the cache: [D, n_kv, kv heads], memory [cell][kv head][row of blocks] */
    cache_view(&K, LFAMD_TYPE_Q8_0, D, N_KV);
    V = K;
    K.view_src = &KC, K.buffer = kvbuf, K.data = KC.data;
    V.view_src = &VC, V.buffer = kvbuf, V.data = VC.data;
    OUT.src[1] = &K, OUT.src[2] = &V;
    struct ggml_tensor *nodes[3] = {&KCPY, &VCPY, &OUT};
    for (int i = 0; i < 3; i++)
        if (!be->iface.supports_op(be, nodes[i])) { fprintf(stderr, "supports_op says no (node %d)\n", i); return 11; }
    struct ggml_cgraph g = {3, 3, 0, nodes, NULL, NULL};
    if (be->iface.graph_compute(be, &g) != GGML_STATUS_SUCCESS) { fprintf(stderr, "graph_compute failed\n"); return 12; }
    be->iface.synchronize(be);
    const size_t no = h_nbytes(&OUT);
    void *ho = malloc(no);
    cbuf->iface.get_tensor(cbuf, &OUT, ho, 0, no);
    dump(argv[9], "", ho, no);
    kvbuf->iface.get_tensor(kvbuf, &KC, hkc, 0, nkc);
    kvbuf->iface.get_tensor(kvbuf, &VC, hvc, 0, nvc);
    dump(argv[10], "", hkc, nkc);
    dump(argv[11], "", hvc, nvc);
    cbuf->iface.free_buffer(cbuf);
    kvbuf->iface.free_buffer(kvbuf);
    be->iface.free(be);
    printf("ok\n");
    return 0;
}

static int faq_run(ggml_backend_t be, ggml_backend_buffer_type_t buft, char **argv) {
    const size_t align = buft->iface.get_alignment(buft);
    const int type = type_of(argv[3]);
    const long n_q = atol(argv[9]), n_kv = atol(argv[10]), mask_rows = atol(argv[11]);
    if (type < 0 || n_q < 1 || n_kv < 1 || mask_rows < n_q) { fprintf(stderr, "usage\n"); return 2; }
    size_t nq, nk, nv, nm;
    void *hq = slurp(argv[4], &nq), *hk = slurp(argv[5], &nk), *hv = slurp(argv[6], &nv), *hm = slurp(argv[7], &nm);
    struct ggml_tensor Q, K, V, M, OUT;
    fa_node(&Q, &K, &V, &M, &OUT, D, type, type, n_q, n_kv, mask_rows);
    if (h_nbytes(&Q) != nq || h_nbytes(&K) != nk || h_nbytes(&V) != nv || h_nbytes(&M) != nm) { fprintf(stderr, "input size mismatch\n"); return 9; }
    ggml_backend_buffer_t kvbuf = buft->iface.alloc_buffer(buft, nk + nv + 8 * align);
    ggml_backend_buffer_t cbuf = buft->iface.alloc_buffer(buft, nq + nm + h_nbytes(&OUT) + 8 * align);
    if (!kvbuf || !cbuf) return 10;
    size_t ko = 2 * align, co = align;
    place(&K, kvbuf, &ko, align);
    place(&V, kvbuf, &ko, align);
    place(&Q, cbuf, &co, align);
    place(&M, cbuf, &co, align);
    place(&OUT, cbuf, &co, align);
    kvbuf->iface.set_tensor(kvbuf, &K, hk, 0, nk);
    kvbuf->iface.set_tensor(kvbuf, &V, hv, 0, nv);
    cbuf->iface.set_tensor(cbuf, &Q, hq, 0, nq);
    cbuf->iface.set_tensor(cbuf, &M, hm, 0, nm);
    struct ggml_tensor *nodes[1] = {&OUT};
    if (!be->iface.supports_op(be, &OUT)) { fprintf(stderr, "supports_op says no\n"); return 11; }
    struct ggml_cgraph g = {1, 1, 0, nodes, NULL, NULL};
    if (be->iface.graph_compute(be, &g) != GGML_STATUS_SUCCESS) { fprintf(stderr, "graph_compute failed\n"); return 12; }
    be->iface.synchronize(be);
    const size_t no = h_nbytes(&OUT);
    void *ho = malloc(no);
    cbuf->iface.get_tensor(cbuf, &OUT, ho, 0, no);
    dump(argv[8], "", ho, no);
    cbuf->iface.free_buffer(cbuf);
    kvbuf->iface.free_buffer(kvbuf);
    be->iface.free(be);
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    api.ggml_op_name = h_op_name_faq;
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
        return argc < 4 ? 2 : faq_decline(be, buft, argv[3]);
    if (!strcmp(argv[2], "store"))
        return argc < 13 ? 2 : faq_store(be, buft, argv);
    if (!strcmp(argv[2], "run"))
        return argc < 12 ? 2 : faq_run(be, buft, argv);
    fprintf(stderr, "unknown mode %s\n", argv[2]);
    return 2;
}
