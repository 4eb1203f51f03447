// split_checks.cpp -- csrc/ndtgpu_split.h on the host, alone: reads one case per line from stdin, writes the header's decision
// per line to stdout (tests/test_split.py compares them exactly; doubles travel as hexadecimal floats, both ways).
//   G maps k n_cu                               -> groups
//   M B M_raw pairs n_cu                        -> proportional chosen
//   P model maps n_cu M_raw clk_per_ms w fail   -> ok groups | the g asked of the probe, in order | the candidates' g
//       (the probe: build_ms(g) = ceil(maps / (4 (n_cu - g))) w; its call number `fail` fails, 0: none)
//   S cells_per_map                             -> slots
//   C n_maps n_results, then n_maps x "cyc0 cyc1 cyc2 cyc3 n_cells" and n_results x "cycles_eval cycles_solver"
//                                               -> B M_raw cells n_bad | per result: sane
//   W new | W calib calib_cells calib_at | W sample cells_per_map depth -> n_recent oldest
//   W ask j depth pct -> yes mean | W measured cells_per_map j -> calib_cells calib_at recal_ref n_recent | W ref recal_ref
#include "../../ndt_feature_graph_amd/csrc/ndtgpu_split.h"

#include <cstdio>
#include <cstring>

static char g_tok[64];
static const char *tok() { if (scanf("%63s", g_tok) != 1) g_tok[0] = 0; return g_tok; }
static double num() { return strtod(tok(), nullptr); }
static long long integer() { return strtoll(tok(), nullptr, 10); }
static bool is(const char *a, const char *b) { return strcmp(a, b) == 0; }

int main()
{
    RecalWindow w;
    for (;;) {
        char op[64];
        strcpy(op, tok());
        if (!op[0]) break;
        if (is(op, "G")) {
            const size_t maps = (size_t)integer();
            const unsigned k = (unsigned)integer();
            printf("%u\n", split_groups_of(maps, k, (int)integer()));
        } else if (is(op, "M")) {
            const double B = num(), M_raw = num();
            const size_t pairs = (size_t)integer();
            const int n_cu = (int)integer();
            printf("%u %u\n", split_proportional(B, M_raw, n_cu), split_model(B, M_raw, pairs, n_cu));
        } else if (is(op, "P")) {
            const unsigned model = (unsigned)integer();
            const size_t maps = (size_t)integer();
            const int n_cu = (int)integer();
            const double M_raw = num(), clk = num(), wg = num();
            const long long fail = integer();
            std::vector<unsigned> asked;
            const SplitSearch s = split_probe_search(model, maps, n_cu, M_raw, clk, [&](unsigned g, double *ms) {
                asked.push_back(g);
                if ((long long)asked.size() == fail) return false;
                *ms = std::ceil((double)maps / (4.0 * (double)(n_cu - (int)g))) * wg;
                return true;
            });
            printf("%d %u |", s.ok ? 1 : 0, s.groups);
            for (unsigned g : asked) printf(" %u", g);
            printf(" |");
            for (const SplitCand &c : s.cand) printf(" %u", c.g);
            printf("\n");
        } else if (is(op, "S")) {
            printf("%d\n", split_slots(num()));
        } else if (is(op, "C")) {
            const size_t n_maps = (size_t)integer(), n_res = (size_t)integer();
            SplitClocks c;
            for (size_t i = 0; i < n_maps; i++) {
                uint32_t cyc[4];
                for (uint32_t &q : cyc) q = (uint32_t)integer();
                c.add_map(cyc, (uint32_t)integer());
            }
            std::vector<int> sane;
            for (size_t i = 0; i < n_res; i++) {
                const long long e = integer(), s = integer();
                sane.push_back(c.add_result(e, s) ? 1 : 0);
            }
            c.finish();
            printf("%a %a %a %zu |", c.B, c.M_raw, c.cells, c.n_bad);
            for (int q : sane) printf(" %d", q);
            printf("\n");
        } else if (is(op, "W")) {
            char what[64];
            strcpy(what, tok());
            if (is(what, "new")) w = RecalWindow();
            else if (is(what, "calib")) { w.calib_cells = num(); w.calib_at = (size_t)integer(); }
            else if (is(what, "ref")) w.recal_ref = num();
            else if (is(what, "sample")) {
                const double v = num();
                w.sample(v, (int)integer());
                printf("%zu %a\n", w.recent.size(), w.recent.front());
            } else if (is(what, "ask")) {
                const size_t j = (size_t)integer();
                const int depth = (int)integer(), pct = (int)integer();
                double mean = -1.0;
                const bool yes = w.should_remeasure(j, depth, pct, &mean);
                printf("%d %a\n", yes ? 1 : 0, mean);
            } else if (is(what, "measured")) {
                const double v = num();
                w.measured(v, (size_t)integer());
                printf("%a %zu %a %zu\n", w.calib_cells, w.calib_at, w.recal_ref, w.recent.size());
            } else { fprintf(stderr, "split_checks: W %s?\n", what); return 2; }
        } else { fprintf(stderr, "split_checks: %s?\n", op); return 2; }
    }
    return 0;
}
