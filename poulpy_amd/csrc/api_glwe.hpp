// api_glwe.hpp — what the C-ABI translation units share above the launch layer: the HIP-graph cache for launch-bound chains and the
// resolution of prepared keys (api.hip).  The batched GLWE product and the composite calls built on it are declared in glwe_call.hpp.
#pragma once
#include "api_common.hpp"

// ------------------------------------------------------------------------------
// HIP graphs for the launch-bound composite calls.  A blind rotation on the composed path is 5 launches per LWE block
// (hundreds per call), a trace 6-8 per step: at small batches the kernels are shorter than their launch cost.  The first
// call with a given argument set runs normally (it sizes the workspaces and builds tables: nothing that allocates or
// synchronizes may happen under capture); the second one is captured on the module's stream and instantiated; from then on
// the call is one hipGraphLaunch.  The key covers every value a kernel argument is derived from (pointers, shapes, the
// module's workspaces and knobs); entries are evicted least-recently-used.  Capture failures fall back to plain launches.
// ------------------------------------------------------------------------------
struct KeyHash {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t len) {
        const unsigned char* c = (const unsigned char*)p;
        for (size_t i = 0; i < len; ++i) { h ^= c[i]; h *= 1099511628211ull; }
    }
    template <typename T> void add(const T& v) { bytes(&v, sizeof(T)); }
};
static void graph_key_module(const pz_module* M, KeyHash& k) {
    k.add(M->ws); k.add(M->ws2); k.add(M->ws_bytes); k.add(M->ws2_bytes); k.add(M->fuse_mid); k.add(M->fuse_tail); k.add(M->small_path); k.add(M->chunk);
    k.add(M->dbg_stages); k.add(M->probe); k.add(M->graph_epoch); k.add(M->w2n);
}
// one tag per call that replays as a graph: two calls with the same arguments never share a key
enum GraphTag : int {
    GRAPH_GLWE_TRACE = 1,             // api_trace.hip
    GRAPH_BLIND_ROTATION = 2,         // api_br.hip
    GRAPH_CIRCUIT_BOOTSTRAPPING = 3,  // api_br.hip
    GRAPH_GLWE_BLIND_ROTATION = 7,    // api_gates.hip
    GRAPH_BLIND_RETRIEVAL = 8,        // api_gates.hip
    GRAPH_BDD_EXECUTE = 9,            // api_bdd.hip
    GRAPH_FHE_UINT_PACK = 11,         // api_fhe_uint.hip
    GRAPH_FHE_UINT_WORD = 12,         // api_fhe_uint.hip
    GRAPH_LINCOMB_CONST = 31,         // api_lincomb.hip (builds its key by hand)
    GRAPH_TENSOR_MUL_ACC = 32,        // api_cnv.hip
    GRAPH_TENSOR_DOT = 33,            // api_cnv.hip (adds every pair's pointers and strides to its key)
};
// the key of a call from its tag, the arguments that are always there, and the module's state; the caller adds what is special to it
template <typename... Args>
static KeyHash graph_key(const pz_module* M, GraphTag tag, const Args&... args) {
    KeyHash k;
    k.add((int)tag);
    (k.add(args), ...);
    graph_key_module(M, k);
    return k;
}
static void graph_drop(pz_module::GraphEntry& e) {
    if (e.exec) (void)hipGraphExecDestroy(e.exec);
    if (e.graph) (void)hipGraphDestroy(e.graph);
    e.exec = nullptr; e.graph = nullptr;
}
template <typename F>
static int with_graph(pz_module* M, uint64_t key, F&& body) {
    static const int env_on = rt_knob("POULPY_DBG_GRAPHS", 1);
    if (!env_on || !M->graphs_on || M->timing || canary_mode()) return body();   // (a replayed graph would not re-arm the workspace guards)
    pz_module::GraphEntry* e = nullptr;
    for (auto& ge : M->graphs) if (ge.key == key) e = &ge;
    if (e && e->exec) {
        e->stamp = ++M->graph_clock;
        PZ_HIP(hipGraphLaunch(e->exec, M->stream));
        M->graph_launches++;
        return PZ_OK;
    }
    if (!e) {  // first sight: plain run, remember the key
        const int rc = body();
        if (rc != PZ_OK) return rc;
        if (M->graphs.size() >= 16) {
            size_t lru = 0;
            for (size_t i = 1; i < M->graphs.size(); ++i) if (M->graphs[i].stamp < M->graphs[lru].stamp) lru = i;
            // the evicted graph may still be executing on the stream, and HIP does not document destroying an executable graph
            // in flight: wait for it (at most one sync per 16 new argument sets)
            if (M->graphs[lru].exec) PZ_HIP(hipStreamSynchronize(M->stream));
            graph_drop(M->graphs[lru]);
            M->graphs.erase(M->graphs.begin() + (long)lru);
        }
        M->graphs.push_back({key, nullptr, nullptr, ++M->graph_clock, false});
        return PZ_OK;
    }
    if (e->failed) return body();
    e->stamp = ++M->graph_clock;
    if (hipStreamBeginCapture(M->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        e->failed = true;
        return body();
    }
    const int rc = body();
    hipGraph_t g = nullptr;
    const hipError_t ce = hipStreamEndCapture(M->stream, &g);
    hipGraphExec_t ex = nullptr;
    if (rc == PZ_OK && ce == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess && ex) {
        // (e may dangle if body() touched M->graphs: it does not — nested calls never go through with_graph)
        e->graph = g; e->exec = ex;
        PZ_HIP(hipGraphLaunch(ex, M->stream));
        M->graph_launches++;
        return PZ_OK;
    }
    (void)hipGetLastError();
    if (g) (void)hipGraphDestroy(g);
    e->failed = true;
    // nothing ran under the failed / invalidated capture (launches issued while capturing only record nodes): run the call plainly,
    // also when body() reported an error that the broken capture itself produced
    return body();
}


// api.hip: drops the device mirror of a host-resident prepared key (a rewritten buffer's mirror would be stale)
int forget_host_key(pz_module* M, const void* host);
void host_key_invalidate(const void* p, size_t bytes);   // api.hip: process-wide (every module's mirrors of that host range)
// api.hip: device pointer of a prepared key - itself when it is one, else its validated (possibly refreshed) device mirror.  A module keeps at most
// kKeyMirrorMax mirrors / kKeyMirrorBytes of them; beyond that the least recently used one is FREED - a call that resolves several host keys must
// not need more of them at once than fit (pz_bdd_circuit_execute_batched checks before it resolves the first one)
constexpr size_t kKeyMirrorMax = 64, kKeyMirrorBytes = (size_t)48 << 30;
int resolve_key(pz_module* M, const double* pmat, size_t bytes, const double** out);
