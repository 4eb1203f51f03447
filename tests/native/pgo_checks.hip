// Direct checks of csrc/ndt_pgo3.h and csrc/ndt_pgo.h: the small functions both pose-graph optimisers and their chip-wide forms
// rest on, one call per case, with nothing of the optimisation around them.
//   pgo_checks <mode> host|gpu      stdin: uint32 n, then n rows of IN[mode] doubles;  stdout: n rows of OUT[mode] doubles
// The per-case body of a table mode is ONE call of the function under test: `host` calls it in a loop, `gpu` from a kernel, one
// thread per case in workgroups of 64 -- both targets run the same source, and tests/test_pgo_direct.py (which builds and drives
// this program) holds both to the same references.  Includes the SE(3) header alone (it brings ndt_pgo.h and ndt_math.h) and links
// only the HIP runtime.  The GPU path makes one launch per run, checks every HIP call, and exits 2 with the error string on the
// first failure.
//
// Table modes (integers travel as doubles; a pose is the header's twelve numbers, a symmetric 6x6 its 21):
//   exp      in  phi (3)                                     out R (9)
//   retract  in  P (12) d (6)                                out Q (12)
//   log      in  R (9)                                       out ok, phi (3), sn, cs
//   linkerr  in  Pi (12) Pj (12) Z (12)                      out ok, e (6), jac (39; NaN wherever link_error stored nothing)
//   jop      in  op side q jac (39) x (6) W (21)             out 6: op 0 pgo3_j(side, jac, x), 1 pgo3_jt(side, jac, x),
//                                                                2 pgo3_j_column(side, jac, q), 3 pgo3_symv(W, x)
//   sym21    in  W36 (36)                                    out W21 (21)
//   tri      in  i j                                         out pgo3_tri(i, j)
//   t16      in  T16 (16)                                    out P by pgo3_from_T16 (12), pgo3_to_T16 of it (16)
//   invsym6  in  C36 (36)                                    out ok, W36 (36)
//   link3    in  T16 (16) has_cov flags cov36 (36)           out Z16 (16) W36 (36)
//   wrap     in  t                                           out ndt_pgo_wrap(t)
//   acos     in  x                                           out ndt_pgo_acos(x)
//   invsym3  in  a b c d e f                                 out ok, W6 (6)
//   link2    in  T16 (16) has_cov flags cov36 (36)           out z3 (3) W6 (6)
// Graph modes, device only (the per-link and per-node bodies are device functions): the "table" is n rows of ONE double, a whole
// graph, which goes through ndt_pgo3_graph / ndt_pgo_graph on a one-graph view whose max_nodes / max_edges exceed N / E.  One
// launch of one workgroup: a thread per link linearises, a barrier, a thread per node gathers (and preconditions), a thread per
// link forms its product, a thread per node sums it.  Before the launch the host checks the counts, the table's length and every
// ref, mov, adj_off and adj entry; a table that fails is refused (exit 65) and nothing is launched.
//   graph3   in  N E max_nodes max_edges, pose (12 N), origin (24), ref (E), mov (E), meas (12 E), info (21 E), prior (21),
//                adj_off (N + 1), adj (2 E), r (6 N), p (6 N)
//            out cost (E + 1), half (E + 1), jac (39 (E + 1)), te after the linearisation (6 (E + 1)), b (6 N), chol (21 N),
//                z = M^-1 r (6 N), te after the link products (6 E), ap (6 N)
//   graph2   in  N E max_nodes max_edges, pose (3 N), origin (3), ref (E), mov (E), meas (3 E), info (6 E), prior (6),
//                adj_off (N + 1), adj (2 E), p (3 N)
//            out cost (E; then the prior's), jac (4 E), te after the linearisation (3 E), b (3 N), dinv (6 N), te after the link
//                products (3 E), ap (3 N)
#include "../../ndt_feature_graph_amd/csrc/ndt_pgo3.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK_HIP(x)                                                                                                    \
    do {                                                                                                                \
        hipError_t e_ = (x);                                                                                            \
        if (e_ != hipSuccess) {                                                                                         \
            fprintf(stderr, "pgo_checks: %s failed: %s\n", #x, hipGetErrorString(e_));                                  \
            exit(2);                                                                                                    \
        }                                                                                                               \
    } while (0)

enum {
    MODE_EXP = 0, MODE_RETRACT, MODE_LOG, MODE_LINKERR, MODE_JOP, MODE_SYM21, MODE_TRI, MODE_T16, MODE_INVSYM6, MODE_LINK3, MODE_WRAP,
    MODE_ACOS, MODE_INVSYM3, MODE_LINK2, N_TABLE_MODES, MODE_GRAPH3 = N_TABLE_MODES, MODE_GRAPH2, N_MODES
};
static const char *const MODE_NAME[N_MODES] = {"exp", "retract", "log", "linkerr", "jop", "sym21", "tri", "t16", "invsym6", "link3", "wrap",
                                               "acos", "invsym3", "link2", "graph3", "graph2"};
static const int MODE_IN[N_MODES] = {3, 18, 9, 36, 69, 36, 2, 16, 36, 54, 1, 1, 6, 54, 1, 1};
static const int MODE_OUT[N_MODES] = {9, 12, 6, 46, 6, 21, 1, 28, 37, 52, 1, 1, 7, 9, 1, 1};
static const unsigned GRAPH_MAX = 4096;          // nodes and links of a graph mode: far above what the checks use

template <int MODE>
NDT_HD void run_case(const double *in, double *out)
{
    if constexpr (MODE == MODE_EXP) {
        pgo3_exp(in, out);
    } else if constexpr (MODE == MODE_RETRACT) {
        pgo3_retract(in, in + 12, out);
    } else if constexpr (MODE == MODE_LOG) {
        out[0] = pgo3_log(in, out + 1, out[4], out[5]) ? 1.0 : 0.0;
    } else if constexpr (MODE == MODE_LINKERR) {
        for (int k = 0; k < NDT_PGO3_JAC; k++) out[7 + k] = NAN;
        out[0] = pgo3_link_error(in, in + 12, in + 24, out + 1, out + 7) ? 1.0 : 0.0;
    } else if constexpr (MODE == MODE_JOP) {
        const int op = (int)in[0], side = in[1] != 0.0 ? 1 : 0;
        int q = (int)in[2];
        q = q < 0 ? 0 : (q > 5 ? 5 : q);
        if (op == 0) pgo3_j(side, in + 3, in + 42, out);
        else if (op == 1) pgo3_jt(side, in + 3, in + 42, out);
        else if (op == 2) pgo3_j_column(side, in + 3, q, out);
        else pgo3_symv(in + 48, in + 42, out);
    } else if constexpr (MODE == MODE_SYM21) {
        pgo3_sym21(in, out);
    } else if constexpr (MODE == MODE_TRI) {
        int i = (int)in[0], j = (int)in[1];
        out[0] = pgo3_tri(i, j);
    } else if constexpr (MODE == MODE_T16) {
        pgo3_from_T16(in, out);
        pgo3_to_T16(out, out + 12);
    } else if constexpr (MODE == MODE_INVSYM6) {
        out[0] = ndt_pgo3_inv_sym6(in, out + 1) ? 1.0 : 0.0;
    } else if constexpr (MODE == MODE_LINK3) {
        ndt_pgo3_link_from_registration(in, in[16] != 0.0 ? in + 18 : nullptr, (int)in[17], out, out + 16);
    } else if constexpr (MODE == MODE_WRAP) {
        out[0] = ndt_pgo_wrap(in[0]);
    } else if constexpr (MODE == MODE_ACOS) {
        out[0] = ndt_pgo_acos(in[0]);
    } else if constexpr (MODE == MODE_INVSYM3) {
        out[0] = ndt_pgo_inv_sym3(in[0], in[1], in[2], in[3], in[4], in[5], out + 1) ? 1.0 : 0.0;
    } else {
        ndt_pgo_link_from_registration(in, in[16] != 0.0 ? in + 18 : nullptr, (int)in[17], out, out + 3);
    }
}

template <int MODE>
__global__ __launch_bounds__(64) void cases_kernel(const double *in, double *out, unsigned n, int n_in, int n_out)
{
    const unsigned k = blockIdx.x * 64u + threadIdx.x;
    if (k >= n) return;
    run_case<MODE>(in + (size_t)k * n_in, out + (size_t)k * n_out);
}

static void need_device()
{
    int n_dev = 0;
    CHECK_HIP(hipGetDeviceCount(&n_dev));
    if (n_dev < 1) {
        fprintf(stderr, "pgo_checks: no HIP device\n");
        exit(3);
    }
}

template <int MODE>
static void run_table(bool gpu, const std::vector<double> &in, std::vector<double> &out, unsigned n)
{
    if (!gpu) {
        for (unsigned k = 0; k < n; k++) run_case<MODE>(in.data() + (size_t)k * MODE_IN[MODE], out.data() + (size_t)k * MODE_OUT[MODE]);
        return;
    }
    need_device();
    double *din = nullptr, *dout = nullptr;
    CHECK_HIP(hipMalloc((void **)&din, in.size() * sizeof(double)));
    CHECK_HIP(hipMalloc((void **)&dout, out.size() * sizeof(double)));
    CHECK_HIP(hipMemcpy(din, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dout, 0xFF, out.size() * sizeof(double)));          // (NaN wherever a case writes nothing)
    hipLaunchKernelGGL((cases_kernel<MODE>), dim3((n + 63u) / 64u), dim3(64), 0, 0, din, dout, n, MODE_IN[MODE], MODE_OUT[MODE]);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipFree(din));
    CHECK_HIP(hipFree(dout));
}

// ---- graph modes ----

// the raw results of one graph, dense (N / E strides), in the order of the mode's output
struct Graph3Out {
    double *cost, *half, *jac, *te_lin, *b, *chol, *z, *te_prod, *ap;
};
struct Graph2Out {
    double *cost, *jac, *te_lin, *b, *dinv, *te_prod, *ap;
};

__global__ __launch_bounds__(64) void graph3_kernel(NdtPgo3View v, NdtPgo3ParamsDev prm, unsigned N, unsigned E, Graph3Out o)
{
    const Pgo3Graph G = ndt_pgo3_graph(v, 0, N, E);
    const unsigned t = threadIdx.x;
    for (unsigned e = t; e <= E; e += 64u) {                                 // (slot E: the prior)
        bool half = false;
        o.cost[e] = pgo3_linearise_link(G, prm, e, half);
        o.half[e] = half ? 1.0 : 0.0;
    }
    __syncthreads();
    for (unsigned k = t; k < NDT_PGO3_JAC * (E + 1); k += 64u) o.jac[k] = G.jac[k];
    for (unsigned k = t; k < 6 * (E + 1); k += 64u) o.te_lin[k] = G.te[k];
    for (unsigned i = t; i < N; i += 64u) pgo3_gather_node(G, prm, i);
    __syncthreads();
    for (unsigned i = t; i < N; i += 64u) {
        double r[6], z[6];
        for (int d = 0; d < 6; d++) r[d] = G.r[6 * (size_t)i + d];
        pgo3_precondition(G, i, r, z);
        for (int d = 0; d < 6; d++) o.z[6 * (size_t)i + d] = z[d];
        for (int d = 0; d < 6; d++) o.b[6 * (size_t)i + d] = G.b[6 * (size_t)i + d];
        for (int d = 0; d < 21; d++) o.chol[21 * (size_t)i + d] = G.chol[21 * (size_t)i + d];
    }
    for (unsigned e = t; e < E; e += 64u) pgo3_link_product(G, e);
    __syncthreads();
    for (unsigned k = t; k < 6 * E; k += 64u) o.te_prod[k] = G.te[k];
    for (unsigned i = t; i < N; i += 64u) {
        double p[6], ap[6];
        for (int d = 0; d < 6; d++) p[d] = G.p[6 * (size_t)i + d];
        pgo3_node_product(G, prm, i, p, ap);
        for (int d = 0; d < 6; d++) o.ap[6 * (size_t)i + d] = ap[d];
    }
}

__global__ __launch_bounds__(64) void graph2_kernel(NdtPgoView v, NdtPgoParamsDev prm, unsigned N, unsigned E, Graph2Out o)
{
    const PgoGraph G = ndt_pgo_graph(v, 0, N, E);
    const unsigned t = threadIdx.x;
    for (unsigned e = t; e < E; e += 64u) o.cost[e] = pgo_linearise_link(G, e);
    if (t == 0) o.cost[E] = pgo_prior_cost(G, prm);
    __syncthreads();
    for (unsigned k = t; k < 4 * E; k += 64u) o.jac[k] = G.jac[k];
    for (unsigned k = t; k < 3 * E; k += 64u) o.te_lin[k] = G.te[k];
    for (unsigned i = t; i < N; i += 64u) pgo_gather_node(G, prm, i);
    __syncthreads();
    for (unsigned i = t; i < N; i += 64u) {
        for (int d = 0; d < 3; d++) o.b[3 * (size_t)i + d] = G.b[3 * (size_t)i + d];
        for (int d = 0; d < 6; d++) o.dinv[6 * (size_t)i + d] = G.dinv[6 * (size_t)i + d];
    }
    for (unsigned e = t; e < E; e += 64u) pgo_link_product(G, e, G.p + 3 * (size_t)G.ref[e], G.p + 3 * (size_t)G.mov[e]);
    __syncthreads();
    for (unsigned k = t; k < 3 * E; k += 64u) o.te_prod[k] = G.te[k];
    for (unsigned i = t; i < N; i += 64u) {
        const double *p = G.p + 3 * (size_t)i;
        pgo_node_product(G, prm, i, p[0], p[1], p[2], o.ap[3 * (size_t)i], o.ap[3 * (size_t)i + 1], o.ap[3 * (size_t)i + 2]);
    }
}

[[noreturn]] static void refuse(const char *mode, const char *what)
{
    fprintf(stderr, "pgo_checks: %s: %s; nothing was launched\n", mode, what);
    exit(65);
}

// a non-negative integer below `limit` that travelled as a double
static bool as_index(double x, double limit, unsigned &out)
{
    if (!(x >= 0.0) || !(x < limit) || x != (double)(unsigned)x) return false;
    out = (unsigned)x;
    return true;
}

// what both graph tables share, checked: the four counts, the total length for `pose_w` doubles per pose, `origin_w` of origin,
// `info_w` per information matrix and `node_w` further doubles per node, and the index arrays
struct GraphTable {
    unsigned N, E, max_nodes, max_edges;
    const double *pose, *origin, *meas, *info, *prior, *node_in;
    std::vector<int32_t> ref, mov;
    std::vector<uint32_t> adj_off, adj;
};

static GraphTable read_graph(const char *mode, const std::vector<double> &in, unsigned pose_w, unsigned origin_w, unsigned info_w,
                             unsigned node_w)
{
    GraphTable T;
    if (in.size() < 4) refuse(mode, "the table has no counts");
    if (!as_index(in[0], GRAPH_MAX + 1.0, T.N) || T.N < 1) refuse(mode, "N is not in 1 .. 4096");
    if (!as_index(in[1], GRAPH_MAX + 1.0, T.E)) refuse(mode, "E is not in 0 .. 4096");
    if (!as_index(in[2], GRAPH_MAX + 1.0, T.max_nodes) || T.max_nodes < T.N) refuse(mode, "max_nodes is not in N .. 4096");
    if (!as_index(in[3], GRAPH_MAX + 1.0, T.max_edges) || T.max_edges < T.E || T.max_edges < 1) refuse(mode, "max_edges is not in max(E, 1) .. 4096");
    const size_t N = T.N, E = T.E;
    const size_t want = 4 + pose_w * N + origin_w + 2 * E + pose_w * E + info_w * E + info_w + (N + 1) + 2 * E + node_w * N;
    if (in.size() != want) refuse(mode, "the table's length does not fit its counts");
    const double *p = in.data() + 4;
    T.pose = p; p += pose_w * N;
    T.origin = p; p += origin_w;
    const double *ref = p; p += E;
    const double *mov = p; p += E;
    T.meas = p; p += pose_w * E;
    T.info = p; p += info_w * E;
    T.prior = p; p += info_w;
    const double *adj_off = p; p += N + 1;
    const double *adj = p; p += 2 * E;
    T.node_in = p;
    T.ref.resize(E); T.mov.resize(E); T.adj_off.resize(N + 1); T.adj.resize(2 * E);
    for (size_t e = 0; e < E; e++) {
        unsigned r, m;
        if (!as_index(ref[e], (double)N, r)) refuse(mode, "a ref entry is not a node");
        if (!as_index(mov[e], (double)N, m)) refuse(mode, "a mov entry is not a node");
        T.ref[e] = (int32_t)r;
        T.mov[e] = (int32_t)m;
    }
    unsigned prev = 0;
    for (size_t i = 0; i <= N; i++) {
        unsigned o;
        if (!as_index(adj_off[i], 2.0 * E + 1.0, o) || o < prev || (i == 0 && o != 0)) refuse(mode, "adj_off does not rise from 0 within 0 .. 2 E");
        T.adj_off[i] = prev = o;
    }
    if (prev != 2 * E) refuse(mode, "adj_off does not end at 2 E");
    for (size_t k = 0; k < 2 * E; k++) {
        unsigned a;
        if (!as_index(adj[k], 2.0 * E, a)) refuse(mode, "an adj entry names no link");
        T.adj[k] = a;
    }
    // (every entry names the link's end the node is: what the bodies assume when they pick a side's Jacobian)
    for (size_t i = 0; i < N; i++)
        for (unsigned k = T.adj_off[i]; k < T.adj_off[i + 1]; k++) {
            const unsigned e = T.adj[k] >> 1;
            if ((unsigned)((T.adj[k] & 1u) ? T.mov[e] : T.ref[e]) != i) refuse(mode, "an adj entry is not one of its node's links");
        }
    return T;
}

template <typename T>
static T *to_device(const void *src, size_t count, size_t room)
{
    T *d = nullptr;
    CHECK_HIP(hipMalloc((void **)&d, room * sizeof(T)));
    CHECK_HIP(hipMemset(d, 0xFF, room * sizeof(T)));                         // (NaN / out-of-range wherever nothing is put)
    if (src && count) CHECK_HIP(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

static std::vector<double> run_graph3(const std::vector<double> &in)
{
    const GraphTable T = read_graph("graph3", in, 12, 24, 21, 12);
    need_device();
    const size_t N = T.N, E = T.E, MN = T.max_nodes, ME = T.max_edges;
    NdtPgo3ParamsDev prm;
    prm.max_iterations = prm.max_linear_iterations = 0;
    prm.eps_step = prm.eps_linear = 0.0;
    for (int k = 0; k < 21; k++) prm.prior[k] = T.prior[k];
    NdtPgo3View v;
    v.max_nodes = MN;
    v.max_edges = ME;
    v.state = nullptr;
    v.pose = to_device<double>(T.pose, 12 * N, 12 * MN);
    v.origin = to_device<double>(T.origin, 24, 24);
    v.ref = to_device<int32_t>(T.ref.data(), E, ME);
    v.mov = to_device<int32_t>(T.mov.data(), E, ME);
    v.meas = to_device<double>(T.meas, 12 * E, 12 * ME);
    v.info = to_device<double>(T.info, 21 * E, 21 * ME);
    v.adj_off = to_device<uint32_t>(T.adj_off.data(), N + 1, MN + 1);
    v.adj = to_device<uint32_t>(T.adj.data(), 2 * E, 2 * ME);
    v.jac = to_device<double>(nullptr, 0, NDT_PGO3_JAC * (ME + 1));
    v.te = to_device<double>(nullptr, 0, 6 * (ME + 1));
    v.node = to_device<double>(nullptr, 0, NDT_PGO3_NODE_DOUBLES * MN);
    // r and p where ndt_pgo3_graph puts them
    CHECK_HIP(hipMemcpy(v.node + 24 * MN, T.node_in, 6 * N * sizeof(double), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(v.node + 36 * MN, T.node_in + 6 * N, 6 * N * sizeof(double), hipMemcpyHostToDevice));
    const size_t n_out = 2 * (E + 1) + 45 * (E + 1) + 6 * N + 21 * N + 6 * N + 6 * E + 6 * N;
    double *dout = to_device<double>(nullptr, 0, n_out);
    Graph3Out o;
    double *p = dout;
    o.cost = p; p += E + 1;
    o.half = p; p += E + 1;
    o.jac = p; p += NDT_PGO3_JAC * (E + 1);
    o.te_lin = p; p += 6 * (E + 1);
    o.b = p; p += 6 * N;
    o.chol = p; p += 21 * N;
    o.z = p; p += 6 * N;
    o.te_prod = p; p += 6 * E;
    o.ap = p;
    hipLaunchKernelGGL(graph3_kernel, dim3(1), dim3(64), 0, 0, v, prm, T.N, T.E, o);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    std::vector<double> out(n_out);
    CHECK_HIP(hipMemcpy(out.data(), dout, n_out * sizeof(double), hipMemcpyDeviceToHost));
    void *all[] = {v.pose, v.origin, v.ref, v.mov, v.meas, v.info, v.adj_off, v.adj, v.jac, v.te, v.node, dout};
    for (void *q : all) CHECK_HIP(hipFree(q));
    return out;
}

static std::vector<double> run_graph2(const std::vector<double> &in)
{
    const GraphTable T = read_graph("graph2", in, 3, 3, 6, 3);
    need_device();
    const size_t N = T.N, E = T.E, MN = T.max_nodes, ME = T.max_edges;
    NdtPgoParamsDev prm;
    prm.max_iterations = prm.max_linear_iterations = 0;
    prm.eps_step = prm.eps_linear = 0.0;
    for (int k = 0; k < 6; k++) prm.prior[k] = T.prior[k];
    NdtPgoView v;
    v.max_nodes = MN;
    v.max_edges = ME;
    v.state = nullptr;
    v.pose = to_device<double>(T.pose, 3 * N, 3 * MN);
    v.origin = to_device<double>(T.origin, 3, 3);
    v.ref = to_device<int32_t>(T.ref.data(), E, ME);
    v.mov = to_device<int32_t>(T.mov.data(), E, ME);
    v.meas = to_device<double>(T.meas, 3 * E, 3 * ME);
    v.info = to_device<double>(T.info, 6 * E, 6 * ME);
    v.adj_off = to_device<uint32_t>(T.adj_off.data(), N + 1, MN + 1);
    v.adj = to_device<uint32_t>(T.adj.data(), 2 * E, 2 * ME);
    v.jac = to_device<double>(nullptr, 0, 4 * ME);
    v.te = to_device<double>(nullptr, 0, 3 * ME);
    v.node = to_device<double>(nullptr, 0, NDT_PGO_NODE_DOUBLES * MN);
    CHECK_HIP(hipMemcpy(v.node + 15 * MN, T.node_in, 3 * N * sizeof(double), hipMemcpyHostToDevice));     // p
    const size_t n_out = (E + 1) + 4 * E + 3 * E + 3 * N + 6 * N + 3 * E + 3 * N;
    double *dout = to_device<double>(nullptr, 0, n_out);
    Graph2Out o;
    double *p = dout;
    o.cost = p; p += E + 1;
    o.jac = p; p += 4 * E;
    o.te_lin = p; p += 3 * E;
    o.b = p; p += 3 * N;
    o.dinv = p; p += 6 * N;
    o.te_prod = p; p += 3 * E;
    o.ap = p;
    hipLaunchKernelGGL(graph2_kernel, dim3(1), dim3(64), 0, 0, v, prm, T.N, T.E, o);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    std::vector<double> out(n_out);
    CHECK_HIP(hipMemcpy(out.data(), dout, n_out * sizeof(double), hipMemcpyDeviceToHost));
    void *all[] = {v.pose, v.origin, v.ref, v.mov, v.meas, v.info, v.adj_off, v.adj, v.jac, v.te, v.node, dout};
    for (void *q : all) CHECK_HIP(hipFree(q));
    return out;
}

int main(int argc, char **argv)
{
    int mode = -1;
    for (int m = 0; m < N_MODES; m++)
        if (argc > 1 && strcmp(argv[1], MODE_NAME[m]) == 0) mode = m;
    const bool gpu = argc > 2 && strcmp(argv[2], "gpu") == 0;
    if (mode < 0 || argc != 3 || (!gpu && strcmp(argv[2], "host") != 0)) {
        fprintf(stderr, "usage: pgo_checks <mode> host|gpu < cases > results\n  modes:");
        for (int m = 0; m < N_MODES; m++) fprintf(stderr, " %s", MODE_NAME[m]);
        fprintf(stderr, "\n");
        return 64;
    }
    if (mode >= N_TABLE_MODES && !gpu) {
        fprintf(stderr, "pgo_checks: %s runs device functions (NDT_D in the headers): there is no host target for it\n", MODE_NAME[mode]);
        return 64;
    }
    unsigned n = 0;
    if (fread(&n, sizeof n, 1, stdin) != 1 || n < 1 || n > (1u << 20)) {
        fprintf(stderr, "pgo_checks: no case count on stdin (1 .. 2^20)\n");
        return 65;
    }
    std::vector<double> in((size_t)n * MODE_IN[mode]), out;
    if (fread(in.data(), sizeof(double), in.size(), stdin) != in.size()) {
        fprintf(stderr, "pgo_checks: %s takes %d doubles per case, the table is short\n", MODE_NAME[mode], MODE_IN[mode]);
        return 65;
    }
    if (mode < N_TABLE_MODES) out.assign((size_t)n * MODE_OUT[mode], 0.0);
    switch (mode) {
    case MODE_EXP: run_table<MODE_EXP>(gpu, in, out, n); break;
    case MODE_RETRACT: run_table<MODE_RETRACT>(gpu, in, out, n); break;
    case MODE_LOG: run_table<MODE_LOG>(gpu, in, out, n); break;
    case MODE_LINKERR: run_table<MODE_LINKERR>(gpu, in, out, n); break;
    case MODE_JOP: run_table<MODE_JOP>(gpu, in, out, n); break;
    case MODE_SYM21: run_table<MODE_SYM21>(gpu, in, out, n); break;
    case MODE_TRI: run_table<MODE_TRI>(gpu, in, out, n); break;
    case MODE_T16: run_table<MODE_T16>(gpu, in, out, n); break;
    case MODE_INVSYM6: run_table<MODE_INVSYM6>(gpu, in, out, n); break;
    case MODE_LINK3: run_table<MODE_LINK3>(gpu, in, out, n); break;
    case MODE_WRAP: run_table<MODE_WRAP>(gpu, in, out, n); break;
    case MODE_ACOS: run_table<MODE_ACOS>(gpu, in, out, n); break;
    case MODE_INVSYM3: run_table<MODE_INVSYM3>(gpu, in, out, n); break;
    case MODE_LINK2: run_table<MODE_LINK2>(gpu, in, out, n); break;
    case MODE_GRAPH3: out = run_graph3(in); break;
    default: out = run_graph2(in); break;
    }
    if (fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size() || fflush(stdout) != 0) return 66;
    return 0;
}
