// ndtgpu_pgo_graph.h -- what the C-ABIs of the two pose-graph optimisers (csrc/ndtgpu_pgo.hip: SE(2); csrc/ndtgpu_pgo3.hip: SE(3))
// do with a graph's shape on the host, whatever its poses are: the checks of set_graph / set_links_device and the node-to-edge
// adjacency the kernels gather over.
#pragma once
#include "ndtgpu_host.h"

#include <numeric>

#pragma GCC visibility push(hidden)

// what set_graph / set_links_device check before the handle is read: indices, self links, every node connected to node 0
inline ndtgpu_status pgo_check_graph(const char *what, size_t n_nodes, const double *pose3, size_t n_edges, const uint32_t *ref_idx,
                                     const uint32_t *mov_idx)
{
    if (n_nodes == 0 || !pose3 || (n_edges && (!ref_idx || !mov_idx)))
        return fail_in(NDTGPU_ERR_INVALID, what, "poses and link indices are required");
    if (n_nodes > (1u << 24) || n_edges > (1u << 27)) return fail_in(NDTGPU_ERR_INVALID, what, "graph too large");
    std::vector<uint32_t> parent(n_nodes);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t a) {
        while (parent[a] != a) {
            parent[a] = parent[parent[a]];
            a = parent[a];
        }
        return a;
    };
    for (size_t e = 0; e < n_edges; e++) {
        if (ref_idx[e] >= n_nodes || mov_idx[e] >= n_nodes) return fail_in(NDTGPU_ERR_INVALID, what, "link index out of range");
        if (ref_idx[e] == mov_idx[e]) return fail_in(NDTGPU_ERR_INVALID, what, "a link joins a node to itself");
        const uint32_t a = find(ref_idx[e]), b = find(mov_idx[e]);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
    for (size_t i = 1; i < n_nodes; i++)
        if (find((uint32_t)i) != 0) return fail_in(NDTGPU_ERR_INVALID, what, "a node is not connected to node 0");
    return NDTGPU_OK;
}

// node -> incident edges, CSR: off [n_nodes + 1], adj [2 n_edges] = (edge << 1) | (1 where the node is the edge's mov), a node's
// entries in ascending edge order
inline void pgo_adjacency(size_t n_nodes, size_t n_edges, const uint32_t *ref_idx, const uint32_t *mov_idx, std::vector<uint32_t> &off,
                          std::vector<uint32_t> &adj)
{
    off.assign(n_nodes + 1, 0);
    adj.resize(2 * n_edges);
    for (size_t e = 0; e < n_edges; e++) {
        off[ref_idx[e] + 1]++;
        off[mov_idx[e] + 1]++;
    }
    for (size_t i = 0; i < n_nodes; i++) off[i + 1] += off[i];
    std::vector<uint32_t> at(off.begin(), off.end() - 1);
    for (size_t e = 0; e < n_edges; e++) {
        adj[at[ref_idx[e]]++] = (uint32_t)(e << 1);
        adj[at[mov_idx[e]]++] = (uint32_t)(e << 1) | 1u;
    }
}

#pragma GCC visibility pop
