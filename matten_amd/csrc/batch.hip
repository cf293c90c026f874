// matten_batch_gather: a training batch assembled on the device from a device-resident set of crystals.
//
// A batch is a disjoint union with node (and edge) ranges in crystal order, so every array of the batch is the
// concatenation of the picked crystals' own rows, some with an offset added: node ids gain the crystal's first node of
// the batch, edge ids (the CSR permutations and row pointers, stored crystal-relative) its first edge.  One launch moves
// everything: the item space is nodes | edges | crystals | one closing item, one thread per item, and a thread walks the
// streams of its class.  The crystal of an item is found by binary search over the destination running sums, which are
// staged in LDS when the batch has at most BATCH_LDS_ROWS - 1 crystals and read from global memory (L2) otherwise.
// No atomics, no workspace, no synchronisation.
//
// matten_batch_gather_padded is the same kernel with PAD = true: the batch grown to fixed sizes (n_nodes, n_edges,
// n_crystals) by padding crystals that the launch synthesises from closed forms: no source array, no search, no second
// launch.  Behind the v_crystals real crystals (v_nodes nodes, v_edges edges: the code path of the plain kernel, which is
// the padded one with no padding crystal) come K = n_crystals - v_crystals >= 1 padding crystals.  Padding crystal 0 owns
// P = n_nodes - v_nodes - (K - 1) >= 1 nodes and all Ep = n_edges - v_edges padding edges, padding crystals 1 .. K-1 one
// node each and no edge.  Node j of padding crystal 0 owns the edges [floor(j Ep / P), floor((j + 1) Ep / P)) (64-bit
// products), each a self-image edge j -> j, so the padding edges are destination-sorted as they stand: both CSR
// permutations are the identity there, both sorted id lists the owner, both row pointers the closed-form bounds.  The
// owner of padding edge q is floor(((q + 1) P - 1) / Ep).  RAW streams get their padding rows from the stream's fill
// (MATTEN_BATCH_PAD_*).
#include "common.h"

constexpr int BATCH_THREADS = 256;
constexpr int BATCH_LDS_ROWS = 1024;   // B + 1 up to this: both running sums in LDS (8 KB)

extern "C" int matten_batch_gather_lds_rows(void) { return BATCH_LDS_ROWS; }
extern "C" int matten_batch_gather_max_streams(void) { return MATTEN_BATCH_MAX_STREAMS; }

// one array of the batch (40 bytes: the 32 of a launch are 1.3 KB of kernel arguments)
struct BatchStream {
    const char* src;
    char* dst;
    int64_t value;   // the fill's element (low 4 bytes for 4-byte elements)
    int32_t row_bytes;
    int16_t cls;   // MATTEN_BATCH_NODE / _EDGE / _CRYSTAL
    int8_t op;     // MATTEN_BATCH_OP_*
    int8_t vec;    // bytes per load / store of a raw row: 4, 8 or 16
    int8_t pad;    // MATTEN_BATCH_PAD_*: the fill of a RAW stream's padding rows
    int8_t elem;   // 4 or 8
};

struct BatchArgs {
    BatchStream s[MATTEN_BATCH_MAX_STREAMS];
    int n_streams;
};

// the real part of a padded batch and where its sizes go (the plain kernel reads none of it: its batch is all real)
struct BatchValid {
    int crystals, nodes, edges;
    int64_t* n_valid;
};

// the last row r of a[0 .. n) with a[r] <= v (a is non-decreasing, a[0] = 0 <= v): crystals without rows are skipped
__device__ __forceinline__ int batch_find(const int32_t* a, int n, int v) {
    int lo = 0, hi = n;   // a[lo] <= v < a[hi] (a[n] = +inf)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void batch_copy_row(char* __restrict__ d, const char* __restrict__ s, int bytes, int vec) {
    if (vec == 16) {
        for (int o = 0; o < bytes; o += 16) *reinterpret_cast<uint4*>(d + o) = *reinterpret_cast<const uint4*>(s + o);
    } else if (vec == 8) {
        for (int o = 0; o < bytes; o += 8) *reinterpret_cast<uint2*>(d + o) = *reinterpret_cast<const uint2*>(s + o);
    } else {
        for (int o = 0; o < bytes; o += 4) *reinterpret_cast<uint32_t*>(d + o) = *reinterpret_cast<const uint32_t*>(s + o);
    }
}

// one real row of one stream from the store's row src_row: the crystal c of the batch starts at node0 / edge0
__device__ __forceinline__ void batch_write_row(const BatchStream& st, int64_t dst_row, int64_t src_row, int c, int node0,
                                                int edge0) {
    switch (st.op) {
    case MATTEN_BATCH_OP_RAW:
        batch_copy_row(st.dst + dst_row * st.row_bytes, st.src + src_row * st.row_bytes, st.row_bytes, st.vec);
        break;
    case MATTEN_BATCH_OP_ADD32_NODE:
        reinterpret_cast<int32_t*>(st.dst)[dst_row] = reinterpret_cast<const int32_t*>(st.src)[src_row] + node0;
        break;
    case MATTEN_BATCH_OP_ADD32_EDGE:
    case MATTEN_BATCH_OP_ROWPTR32:
        reinterpret_cast<int32_t*>(st.dst)[dst_row] = reinterpret_cast<const int32_t*>(st.src)[src_row] + edge0;
        break;
    case MATTEN_BATCH_OP_ADD64_NODE:
        reinterpret_cast<int64_t*>(st.dst)[dst_row] = reinterpret_cast<const int64_t*>(st.src)[src_row] + node0;
        break;
    case MATTEN_BATCH_OP_BATCH64:
        reinterpret_cast<int64_t*>(st.dst)[dst_row] = c;
        break;
    case MATTEN_BATCH_OP_PTR64:
        reinterpret_cast<int64_t*>(st.dst)[dst_row] = node0;
        break;
    }
}

// one padding row of one stream: `owner` is a padding edge's node, [e_lo, e_hi) a padding node's edges (ids of the batch)
__device__ __forceinline__ void batch_write_pad_row(const BatchStream& st, int64_t dst_row, int c, int node0, int64_t owner,
                                                    int64_t e_lo, int64_t e_hi) {
    switch (st.op) {
    case MATTEN_BATCH_OP_RAW: {
        char* d = st.dst + dst_row * st.row_bytes;
        if (st.pad == MATTEN_BATCH_PAD_DEGREE) {
            reinterpret_cast<float*>(d)[0] = (float)(e_hi - e_lo);
            break;
        }
        const int n_elem = st.row_bytes / st.elem;
        for (int e = 0; e < n_elem; ++e) {
            const bool on = st.pad == MATTEN_BATCH_PAD_CONST || (st.pad == MATTEN_BATCH_PAD_FIRST && e == 0) ||
                            (st.pad == MATTEN_BATCH_PAD_DIAG3 && e % 4 == 0);
            const int64_t v = on ? st.value : 0;
            if (st.elem == 8) reinterpret_cast<int64_t*>(d)[e] = v;
            else reinterpret_cast<int32_t*>(d)[e] = (int32_t)v;
        }
        break;
    }
    case MATTEN_BATCH_OP_ADD32_NODE:
        reinterpret_cast<int32_t*>(st.dst)[dst_row] = (int32_t)owner;
        break;
    case MATTEN_BATCH_OP_ADD32_EDGE:
        reinterpret_cast<int32_t*>(st.dst)[dst_row] = (int32_t)dst_row;
        break;
    case MATTEN_BATCH_OP_ROWPTR32:
        reinterpret_cast<int32_t*>(st.dst)[dst_row] = (int32_t)e_lo;
        break;
    case MATTEN_BATCH_OP_ADD64_NODE:
        reinterpret_cast<int64_t*>(st.dst)[dst_row] = owner;
        break;
    case MATTEN_BATCH_OP_BATCH64:
        reinterpret_cast<int64_t*>(st.dst)[dst_row] = c;
        break;
    case MATTEN_BATCH_OP_PTR64:
        reinterpret_cast<int64_t*>(st.dst)[dst_row] = node0;
        break;
    }
}

// table[5][n_crystals + 1] (int32): destination node start, destination edge start, source node start, source edge
// start, source crystal; the closing column holds (n_nodes, n_edges, 0, 0, 0).  PAD: the two destination running sums
// run over the padding crystals too, the closing column holds (n_nodes, n_edges, v_nodes, v_edges, v_crystals) and the
// closing item copies its last three into n_valid.
template <bool LDS, bool PAD>
__global__ __launch_bounds__(BATCH_THREADS) void batch_gather_kernel(const BatchArgs args, const int32_t* __restrict__ table,
                                                                      int n_crystals, int n_nodes, int n_edges,
                                                                      const BatchValid valid) {
    __shared__ int32_t sh[LDS ? 2 * BATCH_LDS_ROWS : 1];
    const int rows = n_crystals + 1;
    if (LDS) {
        for (int k = threadIdx.x; k < 2 * rows; k += BATCH_THREADS) sh[k] = table[k];   // (the two sums are adjacent)
        __syncthreads();
    }
    const int64_t item = (int64_t)blockIdx.x * BATCH_THREADS + threadIdx.x;
    const int64_t total = (int64_t)n_nodes + n_edges + n_crystals + 1;
    if (item >= total) return;

    const int32_t* node_sum = LDS ? sh : table;   // destination running sums: [rows] each
    const int32_t* edge_sum = LDS ? sh + rows : table + rows;
    // the real rows; without padding that is every row, and the search runs over all n_crystals + 1 table rows
    const int v_crystals = PAD ? valid.crystals : n_crystals, v_nodes = PAD ? valid.nodes : n_nodes,
              v_edges = PAD ? valid.edges : n_edges;
    // PAD only, down to e_hi: P and Ep; whether the item is a padding row; a padding edge's node; a padding node's edge
    // range (ids of the batch)
    const int64_t pad_nodes0 = PAD ? (int64_t)n_nodes - v_nodes - (n_crystals - v_crystals - 1) : 0;
    const int64_t pad_edges = PAD ? (int64_t)n_edges - v_edges : 0;
    bool pad = false;
    int64_t owner = 0, e_lo = 0, e_hi = 0;
    int cls, c, local;   // class, crystal of the batch, row inside the crystal
    int64_t dst_row;
    if (item < n_nodes) {
        cls = MATTEN_BATCH_NODE;
        dst_row = item;
        if (!PAD || item < v_nodes) {
            c = batch_find(node_sum, v_crystals + 1, (int)item);
            local = (int)item - node_sum[c];
        } else {
            pad = true;
            const int64_t j = item - v_nodes;
            if (j < pad_nodes0) {
                c = v_crystals;
                local = (int)j;
                e_lo = v_edges + j * pad_edges / pad_nodes0;
                e_hi = v_edges + (j + 1) * pad_edges / pad_nodes0;
            } else {
                c = v_crystals + 1 + (int)(j - pad_nodes0);
                local = 0;
                e_lo = e_hi = n_edges;
            }
        }
    } else if (item < (int64_t)n_nodes + n_edges) {
        cls = MATTEN_BATCH_EDGE;
        dst_row = item - n_nodes;
        if (!PAD || dst_row < v_edges) {
            c = batch_find(edge_sum, v_crystals + 1, (int)dst_row);
            local = (int)dst_row - edge_sum[c];
        } else {
            pad = true;
            c = v_crystals;
            local = (int)(dst_row - v_edges);
            owner = v_nodes + (((int64_t)local + 1) * pad_nodes0 - 1) / pad_edges;   // (pad_edges >= 1: this edge exists)
        }
    } else {
        cls = MATTEN_BATCH_CRYSTAL;
        dst_row = item - n_nodes - n_edges;   // == n_crystals: the closing item
        c = (int)dst_row;
        local = 0;
        pad = PAD && c >= v_crystals;
    }
    const int node0 = node_sum[c], edge0 = edge_sum[c];
    if (c == n_crystals) {
        // closing entries: rowptr[N] = E (both CSRs), ptr[B] = N
        for (int k = 0; k < args.n_streams; ++k) {
            const BatchStream& st = args.s[k];
            if (st.op == MATTEN_BATCH_OP_ROWPTR32) reinterpret_cast<int32_t*>(st.dst)[n_nodes] = n_edges;
            else if (st.op == MATTEN_BATCH_OP_PTR64) reinterpret_cast<int64_t*>(st.dst)[n_crystals] = n_nodes;
        }
        if constexpr (PAD)
            for (int r = 0; r < 3; ++r) valid.n_valid[r] = table[(2 + r) * rows + n_crystals];
        return;
    }
    if (PAD && pad) {
        for (int k = 0; k < args.n_streams; ++k)
            if (args.s[k].cls == cls) batch_write_pad_row(args.s[k], dst_row, c, node0, owner, e_lo, e_hi);
        return;
    }
    const int64_t src_row = cls == MATTEN_BATCH_NODE   ? (int64_t)table[2 * rows + c] + local
                            : cls == MATTEN_BATCH_EDGE ? (int64_t)table[3 * rows + c] + local
                                                       : (int64_t)table[4 * rows + c];
    for (int k = 0; k < args.n_streams; ++k)
        if (args.s[k].cls == cls) batch_write_row(args.s[k], dst_row, src_row, c, node0, edge0);
}

// the stream records of an entry, checked; words = MATTEN_BATCH_STREAM_WORDS: no fill words, the padding rows (which a
// plain batch does not have) zero
static int batch_decode(const int64_t* streams, int64_t n_streams, int words, BatchArgs& args) {
    if (n_streams < 0 || n_streams > MATTEN_BATCH_MAX_STREAMS || (n_streams > 0 && !streams)) return MATTEN_EINVAL;
    const bool has_fill = words == MATTEN_BATCH_PAD_STREAM_WORDS;
    args.n_streams = (int)n_streams;
    for (int k = 0; k < (int)n_streams; ++k) {
        const int64_t* d = streams + (int64_t)k * words;
        const int64_t src = d[0], dst = d[1], elem = d[2], row_elems = d[3], cls = d[4], op = d[5];
        const int64_t pad = has_fill ? d[6] : MATTEN_BATCH_PAD_ZERO, value = has_fill ? d[7] : 0;
        if (elem != 4 && elem != 8) return MATTEN_EINVAL;
        if (row_elems <= 0 || row_elems >= ((int64_t)1 << 28)) return MATTEN_EINVAL;   // (a row stays below 2^31 bytes)
        if (cls != MATTEN_BATCH_NODE && cls != MATTEN_BATCH_EDGE && cls != MATTEN_BATCH_CRYSTAL) return MATTEN_EINVAL;
        if (op < MATTEN_BATCH_OP_RAW || op > MATTEN_BATCH_OP_PTR64) return MATTEN_EINVAL;
        const bool fills = op == MATTEN_BATCH_OP_BATCH64 || op == MATTEN_BATCH_OP_PTR64;
        if (!dst || (!fills && !src)) return MATTEN_EINVAL;
        // the offset forms are one element per row of a fixed width, each in its own class
        const int64_t want_elem = op == MATTEN_BATCH_OP_RAW ? elem
                                  : (op == MATTEN_BATCH_OP_ADD64_NODE || fills) ? 8 : 4;
        if (elem != want_elem || (op != MATTEN_BATCH_OP_RAW && row_elems != 1)) return MATTEN_EINVAL;
        const int64_t want_cls = op == MATTEN_BATCH_OP_RAW ? cls
                                 : (op == MATTEN_BATCH_OP_ROWPTR32 || op == MATTEN_BATCH_OP_BATCH64) ? MATTEN_BATCH_NODE
                                 : op == MATTEN_BATCH_OP_PTR64 ? MATTEN_BATCH_CRYSTAL : MATTEN_BATCH_EDGE;
        if (cls != want_cls) return MATTEN_EINVAL;
        if ((src | dst) % elem) return MATTEN_EINVAL;
        // the fills belong to RAW streams; the degree is one float per node, the diagonal a 3 x 3 row
        if (pad < MATTEN_BATCH_PAD_ZERO || pad > MATTEN_BATCH_PAD_DEGREE) return MATTEN_EINVAL;
        if (op != MATTEN_BATCH_OP_RAW && pad != MATTEN_BATCH_PAD_ZERO) return MATTEN_EINVAL;
        if (pad == MATTEN_BATCH_PAD_DEGREE && (cls != MATTEN_BATCH_NODE || elem != 4 || row_elems != 1)) return MATTEN_EINVAL;
        if (pad == MATTEN_BATCH_PAD_DIAG3 && row_elems != 9) return MATTEN_EINVAL;
        BatchStream& st = args.s[k];
        st.src = (const char*)(uintptr_t)src;
        st.dst = (char*)(uintptr_t)dst;
        st.value = value;
        st.row_bytes = (int32_t)(row_elems * elem);
        st.cls = (int16_t)cls;
        st.op = (int8_t)op;
        const int64_t align = src | dst | st.row_bytes;   // every row of the stream starts on a multiple of `vec`
        st.vec = (int8_t)(align % 16 == 0 ? 16 : align % 8 == 0 ? 8 : 4);
        st.pad = (int8_t)pad;
        st.elem = (int8_t)elem;
    }
    return MATTEN_OK;
}

// the sizes checked (the padded entry has checked valid against them), then the one launch
template <bool PAD>
static int batch_launch(const BatchArgs& args, const int32_t* table, int64_t n_crystals, int64_t n_nodes, int64_t n_edges,
                        const BatchValid& valid, matten_stream_t stream_) {
    if (!table || n_crystals < 0 || n_nodes < 0 || n_edges < 0) return MATTEN_EINVAL;
    if (n_nodes >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31) || n_crystals >= ((int64_t)1 << 31) - 1)
        return MATTEN_EINVAL;
    const int64_t blocks = matten_cdiv(n_nodes + n_edges + n_crystals + 1, BATCH_THREADS);   // (below 2^31: three such sizes)
    const auto kernel = n_crystals + 1 <= BATCH_LDS_ROWS ? batch_gather_kernel<true, PAD> : batch_gather_kernel<false, PAD>;
    kernel<<<(unsigned)blocks, BATCH_THREADS, 0, (hipStream_t)stream_>>>(args, table, (int)n_crystals, (int)n_nodes,
                                                                          (int)n_edges, valid);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_batch_gather(const int64_t* streams, int64_t n_streams, const int32_t* table, int64_t n_crystals,
                                   int64_t n_nodes, int64_t n_edges, matten_stream_t stream) {
    BatchArgs args;
    if (batch_decode(streams, n_streams, MATTEN_BATCH_STREAM_WORDS, args) != MATTEN_OK) return MATTEN_EINVAL;
    return batch_launch<false>(args, table, n_crystals, n_nodes, n_edges, BatchValid{}, stream);
}

extern "C" int matten_batch_gather_padded(const int64_t* streams, int64_t n_streams, const int32_t* table,
                                          int64_t n_crystals, int64_t n_nodes, int64_t n_edges, int64_t v_crystals,
                                          int64_t v_nodes, int64_t v_edges, int64_t* n_valid, matten_stream_t stream) {
    if (v_crystals < 0 || v_nodes < 0 || v_edges < 0 || !n_valid) return MATTEN_EINVAL;
    // at least one padding crystal, at least one node in the first of them, one node in each of the others
    if (n_crystals <= v_crystals || n_edges < v_edges || n_nodes < v_nodes + (n_crystals - v_crystals)) return MATTEN_EINVAL;
    BatchArgs args;
    if (batch_decode(streams, n_streams, MATTEN_BATCH_PAD_STREAM_WORDS, args) != MATTEN_OK) return MATTEN_EINVAL;
    // (the valid sizes fit an int: the launch refuses n_* of 2^31 or more before it starts anything)
    return batch_launch<true>(args, table, n_crystals, n_nodes, n_edges,
                              BatchValid{(int)v_crystals, (int)v_nodes, (int)v_edges, n_valid}, stream);
}
