// linkgate_checks.hip -- csrc/ndt_linkgate.h on the HOST: reads one case per line from stdin and writes what the header computes
// (tests/test_linkgate_header.py compares it exactly with tests/linkgate_model.py; doubles travel as hexadecimal floats, both ways).
//   D clip p1[16] p2[16]   -> dist ang                                     (poses column-major, as everywhere)
//   C R[16] L[16]          -> the 16 entries of ndt_linkgate_compose
//   R Ti[16] Tj[16]        -> the 16 entries of ndt_linkgate_relative
//   P p n                  -> i j of ndt_linkgate_decode_pair
//   V n_nodes nodes[16 n] ref mov T[16] has_score score max_score max_dist max_angle min_idx_dist clip -> 0 / 1
#include "../../ndt_feature_graph_amd/csrc/ndt_linkgate.h"

#include <cstdio>
#include <cstring>
#include <vector>

static char g_tok[64];
static const char *tok() { if (scanf("%63s", g_tok) != 1) g_tok[0] = 0; return g_tok; }
static double num() { return strtod(tok(), nullptr); }
static long long integer() { return strtoll(tok(), nullptr, 10); }
static void pose(double *T) { for (int k = 0; k < 16; k++) T[k] = num(); }

int main()
{
    for (;;) {
        char op[64];
        strcpy(op, tok());
        if (!op[0]) break;
        double a[16], b[16], out[16];
        if (op[0] == 'D') {
            const int clip = (int)integer();
            pose(a); pose(b);
            double dist, ang;
            ndt_linkgate_distance(a, b, clip, dist, ang);
            printf("%a %a\n", dist, ang);
        } else if (op[0] == 'C' || op[0] == 'R') {
            pose(a); pose(b);
            if (op[0] == 'C') ndt_linkgate_compose(a, b, out); else ndt_linkgate_relative(a, b, out);
            for (int k = 0; k < 16; k++) printf("%a%c", out[k], k == 15 ? '\n' : ' ');
        } else if (op[0] == 'P') {
            const uint64_t p = (uint64_t)integer();
            const uint32_t n = (uint32_t)integer();
            uint32_t i, j;
            ndt_linkgate_decode_pair(p, n, i, j);
            printf("%u %u\n", i, j);
        } else if (op[0] == 'V') {
            const uint32_t n = (uint32_t)integer();
            std::vector<double> nodes(16 * (size_t)n);
            for (double &v : nodes) v = num();
            const uint32_t ref = (uint32_t)integer(), mov = (uint32_t)integer();
            pose(a);
            const int has_score = (int)integer();
            const double score = num();
            NdtLinkGateParamsDev prm;
            prm.max_score = num(); prm.max_dist = num(); prm.max_angle = num();
            prm.min_idx_dist = (int)integer(); prm.clip_cosine = (int)integer();
            printf("%d\n", ndt_linkgate_link_valid(nodes.data(), n, ref, mov, a, has_score ? &score : nullptr, prm) ? 1 : 0);
        } else {
            fprintf(stderr, "unknown case %s\n", op);
            return 2;
        }
    }
    return 0;
}
