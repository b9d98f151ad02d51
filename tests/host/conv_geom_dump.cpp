// Prints every geometry descriptor the conv entry points hand to the kernels, for a fixed problem list: one line per
// descriptor, "<label> <bytes of the struct in hex>".  tests/test_conv_geom_host.py compares the output with
// tests/golden/conv_geom.txt (recorded from the builders as they stood inside conv.hip before they moved to conv_geom.h).
#include "conv_geom.h"

#include <stdio.h>

using namespace mvd;

template <class G>
static void dump(const char *what, const char *problem, const G &g) {
    printf("%s %s ", what, problem);
    const unsigned char *b = reinterpret_cast<const unsigned char *>(&g);
    for (size_t i = 0; i < sizeof(g); i++) printf("%02x", b[i]);
    printf("\n");
}

int main() {
    const int KS[4][3] = {{3, 3, 3}, {1, 3, 3}, {3, 3, 1}, {1, 1, 1}};
    const int ST[3][3] = {{1, 1, 1}, {2, 2, 2}, {1, 2, 2}};
    const int DIMS[2][3] = {{5, 6, 7}, {8, 8, 8}};
    const int CH[2][3] = {{4, 0, 32}, {32, 64, 96}};  // C1, C2, K
    const int N = 2;
    char problem[160], what[64];
    FwdGeom f;
    WgradGeom w;
    for (const auto &ks : KS)
        for (const auto &st : ST)
            for (const auto &d : DIMS)
                for (const auto &c : CH) {
                    snprintf(problem, sizeof(problem), "k%d%d%d s%d%d%d %dx%dx%d c%d+%d k%d", ks[0], ks[1], ks[2], st[0], st[1],
                             st[2], d[0], d[1], d[2], c[0], c[1], c[2]);
                    conv_fwd_geom(f, N, d[0], d[1], d[2], c[0], c[1], c[2], ks, st);
                    dump("conv_fwd", problem, f);
                    for (int pd = 0; pd < st[0]; pd++)
                        for (int ph = 0; ph < st[1]; ph++)
                            for (int pw = 0; pw < st[2]; pw++) {
                                const int p[3] = {pd, ph, pw};
                                snprintf(what, sizeof(what), "conv_dgrad[%d%d%d]", pd, ph, pw);
                                if (conv_dgrad_class_geom(f, N, d[0], d[1], d[2], c[0], c[1], c[2], ks, st, p))
                                    dump(what, problem, f);
                                else
                                    printf("%s %s none\n", what, problem);
                            }
                    conv_wgrad_geom(w, N, d[0], d[1], d[2], c[0], c[1], c[2], ks, st);
                    dump("conv_wgrad", problem, w);
                }
    // a volume with an empty parity class (extent 1 along a stride-2 axis)
    {
        const int ks[3] = {3, 3, 3}, st[3] = {2, 2, 2};
        for (int pd = 0; pd < 2; pd++)
            for (int ph = 0; ph < 2; ph++)
                for (int pw = 0; pw < 2; pw++) {
                    const int p[3] = {pd, ph, pw};
                    snprintf(what, sizeof(what), "conv_dgrad[%d%d%d]", pd, ph, pw);
                    if (conv_dgrad_class_geom(f, N, 1, 4, 1, 32, 0, 32, ks, st, p))
                        dump(what, "k333 s222 1x4x1 c32+0 k32", f);
                    else
                        printf("%s %s none\n", what, "k333 s222 1x4x1 c32+0 k32");
                }
    }
    for (int si = 1; si < 3; si++)
        for (const auto &d : DIMS) {
            const int *st = ST[si];
            snprintf(problem, sizeof(problem), "s%d%d%d %dx%dx%d c64 k32", st[0], st[1], st[2], d[0], d[1], d[2]);
            for (int pd = 0; pd < st[0]; pd++)
                for (int ph = 0; ph < st[1]; ph++)
                    for (int pw = 0; pw < st[2]; pw++) {
                        const int p[3] = {pd, ph, pw};
                        snprintf(what, sizeof(what), "convT_fwd[%d%d%d]", pd, ph, pw);
                        convT_fwd_class_geom(f, N, d[0], d[1], d[2], 64, 32, st, p);
                        dump(what, problem, f);
                    }
            convT_dgrad_geom(f, N, d[0], d[1], d[2], 64, 32, st);
            dump("convT_dgrad", problem, f);
            convT_wgrad_geom(w, N, d[0], d[1], d[2], 64, 32, st);
            dump("convT_wgrad", problem, w);
        }
    return 0;
}
