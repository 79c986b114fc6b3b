/*
 * backend_host_iq4nl.c — TEST INFRASTRUCTURE: backend_host.c as a host whose type table names ggml type 20 "iq4_nl", the way a
 * ggml build that has the type does.  backend_host.c itself stands for a host built before the type existed (its table answers
 * "?" for 20), which the module links with and declines IQ4_NL for; this one is served.  Same command line.
 */
#define main backend_host_main
#include "backend_host.c"
#undef main

static GGML_CALL const char *h_type_name_iq4nl(int t) { return t == LFAMD_TYPE_IQ4_NL ? "iq4_nl" : h_type_name(t); }

int main(int argc, char **argv) {
    api.ggml_type_name = h_type_name_iq4nl;
    return backend_host_main(argc, argv);
}
