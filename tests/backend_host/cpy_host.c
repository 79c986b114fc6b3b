/*
 * cpy_host.c — TEST INFRASTRUCTURE: backend_host.c's host side for GGML_OP_CPY into a K / V cache in the module's buffers.  Its
 * operator table names CPY (and FLASH_ATTN_EXT) at numbers that are not upstream's (the module must find them by name), or —
 * CPY_HOST_NO_NAME=1 — names no CPY at all: the module then links and is never offered the node.
 *
 *   cpy_host <module.so> decline <case>   what supports_op says for one node ("accepted" / "declined"); nothing is computed.
 *       control (F32 [128, 2, 3] into a Q8_0 1-D view of a cache, at cell 5), control_f16, control_move (Q8_0 onto Q8_0), dst_q6_k,
 *       src_f16_dst_f32, nelements (the view one block short), ne0_32 (rows of 48), strided_src (source elements 8 bytes apart, block
 *       destination), view_offs_odd (the view 35 bytes into the cache, no address yet), control_view_offs (34 bytes in, no address yet)
 *   cpy_host <module.so> store <k_cache> <v_cache> <k_cur> <v_cur> <Q> <mask> <out> <k_cache out> <v_cache out>
 *       ONE graph_compute of three nodes on an F16 cache of 8 cells of 2 KV heads x 128 (the files hold its first contents, whole):
 *       CPY of k_cur (F32 [128, 2, 1]) into cell 5 of K, CPY of v_cur (F32 [256, 1]) into cell 5 of V (rows, the -fa layout), then
 *       FLASH_ATTN_EXT of 8 heads, one query, over cells 0 .. 5 (mask F16 [6 x 32]); the result and both caches are read back
 *   cpy_host <module.so> kq8 <k_cur> <n_tok> <k_cache out>
 *       one graph with a Q8_0 K store: k_cur F32 [128, 2, n_tok] into cells 2 .. of a Q8_0 cache of 8 cells that held the byte pattern
 *       (37 i + 11) % 251; the cache is read back with get_tensor
 */
#include <math.h>

#define main backend_host_main
#include "backend_host.c"
#undef main

#define OP_FLASH_ATTN_EXT 47 /* (upstream's numbers differ) */
#define OP_CPY 52

static GGML_CALL const char *h_op_name_cpy(int op) {
    if (op == OP_CPY && !getenv("CPY_HOST_NO_NAME"))
        return "CPY";
    if (op == OP_FLASH_ATTN_EXT)
        return "FLASH_ATTN_EXT";
    return op >= 0 && op < 60 ? h_op_name(op) : NULL; /* a table of 60 names */
}

enum { D = 128, KVH = 2, HEADS = 8, N_CTX = 8, HEAD = 5, N_KV = 6, N_Q = 1, MASK_ROWS = 32, WIDTH = D * KVH };

/* dst: a 1-D view of n elements, `offs` bytes into the cache tensor; node: the CPY of src into it (itself a view of dst) */
static void cpy_node(struct ggml_tensor *node, struct ggml_tensor *dst, struct ggml_tensor *src, struct ggml_tensor *cache, int64_t n, size_t offs) {
    shape(dst, cache->type, n, 1, 1, 1);
    dst->view_src = cache, dst->view_offs = offs, dst->buffer = cache->buffer, dst->data = cache->data ? (uint8_t *)cache->data + offs : NULL;
    *node = *dst;
    node->op = OP_CPY, node->src[0] = src, node->src[1] = dst;
}

static int cpy_decline(ggml_backend_t be, ggml_backend_buffer_type_t buft, const char *what) {
    const size_t align = buft->iface.get_alignment(buft);
    ggml_backend_buffer_t buf = buft->iface.alloc_buffer(buft, 1 << 20);
    if (!buf) return 10;
    const bool move = !strcmp(what, "control_move");
    const int ctype = !strcmp(what, "dst_q6_k") ? LFAMD_TYPE_Q6_K : !strcmp(what, "control_f16") ? LFAMD_TYPE_F16
                      : !strcmp(what, "src_f16_dst_f32") ? LFAMD_TYPE_F32 : LFAMD_TYPE_Q8_0;
    const int stype = !strcmp(what, "src_f16_dst_f32") ? LFAMD_TYPE_F16 : move ? LFAMD_TYPE_Q8_0 : LFAMD_TYPE_F32;
    struct ggml_tensor CACHE, SRC, DST, NODE;
    shape(&CACHE, ctype, (int64_t)WIDTH * N_CTX, 1, 1, 1);
    if (!strcmp(what, "ne0_32"))
        shape(&SRC, stype, 48, 16, 1, 1);
    else if (move)
        shape(&SRC, stype, WIDTH * 3, 1, 1, 1);
    else
        shape(&SRC, stype, D, KVH, 3, 1);
    size_t off = align;
    place(&CACHE, buf, &off, align);
    place(&SRC, buf, &off, align);
    const size_t row = CACHE.nb[0] * WIDTH / lfamd_blck_size(ctype);
    cpy_node(&NODE, &DST, &SRC, &CACHE, WIDTH * 3, HEAD * row);
    if (!strcmp(what, "control") || !strcmp(what, "control_f16") || move || !strcmp(what, "dst_q6_k") || !strcmp(what, "src_f16_dst_f32")) {
        /* (the node as built) */
    } else if (!strcmp(what, "nelements")) {
        DST.ne[0] -= 32, NODE.ne[0] -= 32;
    } else if (!strcmp(what, "ne0_32")) {
        /* (768 elements in rows of 48) */
    } else if (!strcmp(what, "strided_src")) {
        SRC.nb[0] = 8; /* every other float of a wider tensor */
    } else if (!strcmp(what, "view_offs_odd") || !strcmp(what, "control_view_offs")) {
        DST.view_offs = NODE.view_offs = !strcmp(what, "view_offs_odd") ? 35 : 34, DST.data = NODE.data = NULL;
    } else {
        fprintf(stderr, "unknown case %s\n", what);
        return 2;
    }
    printf("%s\n", be->iface.supports_op(be, &NODE) ? "accepted" : "declined");
    buf->iface.free_buffer(buf);
    be->iface.free(be);
    return 0;
}

static int cpy_store(ggml_backend_t be, ggml_backend_buffer_type_t buft, char **argv) {
    const size_t align = buft->iface.get_alignment(buft);
    size_t nkc, nvc, nk, nv, nq, nm;
    void *hkc = slurp(argv[3], &nkc), *hvc = slurp(argv[4], &nvc), *hk = slurp(argv[5], &nk), *hv = slurp(argv[6], &nv);
    void *hq = slurp(argv[7], &nq), *hm = slurp(argv[8], &nm);
    struct ggml_tensor KC, VC, KCUR, VCUR, KDST, VDST, KCPY, VCPY, Q, K, V, M, OUT;
    shape(&KC, LFAMD_TYPE_F16, (int64_t)WIDTH * N_CTX, 1, 1, 1);
    shape(&VC, LFAMD_TYPE_F16, (int64_t)WIDTH * N_CTX, 1, 1, 1);
    shape(&KCUR, LFAMD_TYPE_F32, D, KVH, 1, 1);
    shape(&VCUR, LFAMD_TYPE_F32, WIDTH, 1, 1, 1);
    shape(&Q, LFAMD_TYPE_F32, D, N_Q, HEADS, 1); /* memory [n_q][heads][D] */
    Q.nb[1] = (size_t)HEADS * D * 4, Q.nb[2] = (size_t)D * 4, Q.nb[3] = (size_t)N_Q * HEADS * D * 4;
    shape(&M, LFAMD_TYPE_F16, N_KV, MASK_ROWS, 1, 1);
    shape(&OUT, LFAMD_TYPE_F32, D, HEADS, N_Q, 1);
    if (h_nbytes(&KC) != nkc || h_nbytes(&VC) != nvc || h_nbytes(&KCUR) != nk || h_nbytes(&VCUR) != nv || h_nbytes(&Q) != nq || h_nbytes(&M) != nm) {
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
    cpy_node(&KCPY, &KDST, &KCUR, &KC, WIDTH, (size_t)HEAD * WIDTH * 2);
    cpy_node(&VCPY, &VDST, &VCUR, &VC, WIDTH, (size_t)HEAD * WIDTH * 2);
    /* the attention's views of the cache: [D, n_kv, kv heads], memory [cell][kv head][D] */
    shape(&K, LFAMD_TYPE_F16, D, N_KV, KVH, 1);
    K.nb[1] = (size_t)WIDTH * 2, K.nb[2] = (size_t)D * 2, K.nb[3] = (size_t)N_KV * WIDTH * 2;
    V = K;
    K.view_src = &KC, K.buffer = kvbuf, K.data = KC.data;
    V.view_src = &VC, V.buffer = kvbuf, V.data = VC.data;
    const float scale = 1.0f / sqrtf((float)D), max_bias = 0.0f;
    memcpy(&OUT.op_params[0], &scale, 4);
    memcpy(&OUT.op_params[1], &max_bias, 4);
    OUT.op_params[2] = 0; /* GGML_PREC_DEFAULT */
    OUT.op = OP_FLASH_ATTN_EXT, OUT.src[0] = &Q, OUT.src[1] = &K, OUT.src[2] = &V, OUT.src[3] = &M;
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

static int cpy_kq8(ggml_backend_t be, ggml_backend_buffer_type_t buft, char **argv) {
    const size_t align = buft->iface.get_alignment(buft);
    const long n_tok = atol(argv[4]);
    size_t nk;
    void *hk = slurp(argv[3], &nk);
    struct ggml_tensor KC, KCUR, KDST, KCPY;
    shape(&KC, LFAMD_TYPE_Q8_0, (int64_t)WIDTH * N_CTX, 1, 1, 1);
    shape(&KCUR, LFAMD_TYPE_F32, D, KVH, n_tok, 1);
    if (n_tok < 1 || 2 + n_tok > N_CTX || h_nbytes(&KCUR) != nk) { fprintf(stderr, "input size mismatch\n"); return 9; }
    const size_t nkc = h_nbytes(&KC), row = nkc / N_CTX;
    uint8_t *hkc = malloc(nkc);
    for (size_t i = 0; i < nkc; i++)
        hkc[i] = (uint8_t)((i * 37 + 11) % 251);
    ggml_backend_buffer_t kvbuf = buft->iface.alloc_buffer(buft, nkc + 8 * align);
    ggml_backend_buffer_t cbuf = buft->iface.alloc_buffer(buft, nk + 8 * align);
    if (!kvbuf || !cbuf) return 10;
    size_t ko = 2 * align, co = align;
    place(&KC, kvbuf, &ko, align);
    place(&KCUR, cbuf, &co, align);
    kvbuf->iface.set_tensor(kvbuf, &KC, hkc, 0, nkc);
    cbuf->iface.set_tensor(cbuf, &KCUR, hk, 0, nk);
    cpy_node(&KCPY, &KDST, &KCUR, &KC, (int64_t)WIDTH * n_tok, 2 * row);
    struct ggml_tensor *nodes[1] = {&KCPY};
    if (!be->iface.supports_op(be, &KCPY)) { fprintf(stderr, "supports_op says no\n"); return 11; }
    struct ggml_cgraph g = {1, 1, 0, nodes, NULL, NULL};
    if (be->iface.graph_compute(be, &g) != GGML_STATUS_SUCCESS) { fprintf(stderr, "graph_compute failed\n"); return 12; }
    be->iface.synchronize(be);
    kvbuf->iface.get_tensor(kvbuf, &KC, hkc, 0, nkc);
    dump(argv[5], "", hkc, nkc);
    cbuf->iface.free_buffer(cbuf);
    kvbuf->iface.free_buffer(kvbuf);
    be->iface.free(be);
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    api.ggml_op_name = h_op_name_cpy;
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
        return argc < 4 ? 2 : cpy_decline(be, buft, argv[3]);
    if (!strcmp(argv[2], "store"))
        return argc < 12 ? 2 : cpy_store(be, buft, argv);
    if (!strcmp(argv[2], "kq8"))
        return argc < 6 ? 2 : cpy_kq8(be, buft, argv);
    fprintf(stderr, "unknown mode %s\n", argv[2]);
    return 2;
}
