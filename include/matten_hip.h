/*
 * matten_hip.h -- C ABI of libmatten_hip.so: MI355X (gfx950) kernels for MatTen's equivariant
 * message-passing hot path.
 *
 * The reference (wengroup/matten) has no FFI for this path: it calls e3nn / torch_scatter Python
 * ops.  Each entry point below replaces one of those call sites (cited as reference file:line,
 * relative to the reference repository root) and is what a ctypes / pybind stub on the reference
 * side would bind -- see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch); no allocation inside
 *   - kernels are enqueued on `stream` and never synchronise; the library keeps no global state
 *   - return value: 0 on success, negative MATTEN_E* on a host-detectable error
 *     (data-dependent errors, e.g. an unsupported atomic number, are reported through a device
 *     `int32_t* err_flag` the caller reads back when it wants to)
 *   - fp32 data, int32 indices inside the library; the backbone boundary's int64 tensors
 *     (edge_index, atomic_numbers, batch, ptr -- reference data/_dtype.py:4) are read as int64
 *   - irreps data layout: blocks concatenated, each block [mul, 2l+1] row-major (e3nn "mul_ir")
 */
#ifndef MATTEN_HIP_H
#define MATTEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* matten_stream_t; /* hipStream_t */

#define MATTEN_OK 0
#define MATTEN_EINVAL (-1)  /* bad argument (null pointer, negative size, unsupported shape) */
#define MATTEN_ELAUNCH (-2) /* hipGetLastError() != hipSuccess after a launch */
#define MATTEN_ENOMEM (-3)  /* caller-provided workspace too small */

/* ABI version of this header; bumped on any signature change (47: open / partly periodic graph prologue, pair-free neighbour search). */
int matten_abi_version(void);

/* Radial MLP depth.  The reference builds every conv layer's radial network as FullyConnectedNet([nb] + L x [32] + [W],
 * silu) with L = invariant_layers (nn/utils.py:244-251).  The entries without a suffix take the L = 2 shape (w1p, one
 * middle layer); each has a _deep sibling that takes (w_mid, n_mid) in place of w1p / w1: n_mid = L - 1 middle layers
 * 32 -> 32 (silu), their weights ONE buffer w_mid[n_mid][32][32] (packed: each pre-scaled like w1p; raw: like w1), NULL
 * allowed for n_mid = 0.  n_mid outside 0..MATTEN_RADIAL_MAX_MID is MATTEN_EINVAL.  n_mid = 1 runs the same kernels as
 * the unsuffixed entry. */
#define MATTEN_RADIAL_MAX_MID 3

/* ------------------------------------------------------------------------------------------
 * Graph indexing.  Replaces the implicit ordering torch_scatter.scatter(msg, edge_dst) relies
 * on (nn/conv.py:113-114): builds a destination-sorted CSR so that the neighbour sum is a
 * segmented reduction with a fixed (stable => deterministic) summation order.
 *   edge_index [2,E] int64: row 0 = centre i ("src"), row 1 = neighbour j ("dst") -- data/data.py:297-301
 *   perm[E]      : sorted position -> original edge id (stable sort by dst)
 *   rowptr[N+1]  : CSR offsets into the sorted edge list
 *   src_sorted[E]: edge_index[0][perm[e]]
 * workspace: matten_csr_workspace_bytes(E, N) bytes.
 * Out-of-range node ids set err_flag bit 0.
 * Sparse graphs (E <= 64 N) are built by counting (in-degree atomics, scan, rank of the edge ids inside every
 * segment: no device-wide sort), dense ones by a stable radix sort; the result is the same.  The ranking step costs
 * degree^2 / 16 comparisons per node (cutoff-radius graphs: degree ~ 10-200); a hub segment of more than 2048 edges in
 * an otherwise sparse graph is sorted by a whole workgroup instead (O(d log^2 d), same order).
 * ------------------------------------------------------------------------------------------ */
size_t matten_csr_workspace_bytes(int64_t n_edges, int64_t n_nodes);
int matten_csr_counting_max_avg_degree(void);   /* E <= this * N: counting build (no device-wide sort) */
int matten_csr_build(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, int32_t* perm,
                     int32_t* rowptr, int32_t* src_sorted, void* workspace, size_t workspace_bytes,
                     int32_t* err_flag, matten_stream_t stream);

/* Long CSR segments cut into VIRTUAL nodes of at most max_len edges (small batches, where one hub -- a one-atom cell has
 * hundreds of neighbours inside the cutoff -- would otherwise set the duration of every tensor-product launch: the kernels
 * walk a segment serially).  The pieces tile the sorted edge list in order:
 *   vrowptr[bound + 1] : CSR row pointer over virtual nodes (pieces past the real count are empty, = n_edges)
 *   vseg[n_nodes + 1]  : int64, virtual range of every real node (the `ptr` of matten_segment_reduce: the real node's
 *                        neighbour sum = ordered sum of its pieces' rows)
 *   vnn[bound]         : num_neigh of the piece's real node (optional, for per-node normalisation; both NULL or neither)
 * bound = matten_csr_split_bound(n_nodes, n_edges, max_len) = n_nodes + n_edges / max_len; no host sync.
 * Reference: the order torch_scatter.scatter adds messages in is unspecified (nn/conv.py:114); here it is fixed and
 * depends on the node's own segment only. */
int64_t matten_csr_split_bound(int64_t n_nodes, int64_t n_edges, int64_t max_len);
int matten_csr_split(const int32_t* rowptr, int64_t n_nodes, int64_t n_edges, int64_t max_len, int32_t* vrowptr,
                     int64_t* vseg, const float* num_neigh, float* vnn, matten_stream_t stream);

/* Grouping of n items by an integer key in [0, n_keys): order[n] = item positions stably sorted by key,
 * seg[n_keys+1] = first sorted position of each key.  This is the species grouping the species-indexed linears
 * (FullyConnectedTensorProduct with a one-hot operand, nn/conv.py:59-86) walk instead of evaluating densely over
 * the one-hot.  workspace: matten_group_workspace_bytes(n, n_keys) bytes.  A key out of range sets err_flag bit 0.
 * (n_keys <= 256: per-run histograms + scan + ballot ranks; more keys: stable radix sort.) */
size_t matten_group_workspace_bytes(int64_t n, int64_t n_keys);
int matten_group_by_key(const int64_t* key, int64_t n, int64_t n_keys, int32_t* order, int32_t* seg,
                        void* workspace, size_t workspace_bytes, int32_t* err_flag, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SpeciesEmbedding.forward (nn/embedding.py:85-110) + _AtomicNumberToIndex.forward (:230-259)
 *   species_index[n] = z_to_index[Z[n] - min_z]           (int64 out, reference dtype)
 *   node_feats[n,:]  = W[:, species] + b                   (Linear on a one-hot == column lookup)
 *   node_attrs (one-hot [N,S]) is written only if node_attrs != NULL.
 * err_flag bit 1: Z outside [min_z,max_z]; bit 2: Z maps to -1 (unsupported species).
 * ------------------------------------------------------------------------------------------ */
int matten_species_embed(const int64_t* atomic_numbers, int64_t n_nodes, const int64_t* z_to_index,
                         int64_t min_z, int64_t max_z, int64_t n_species, const float* weight /*[dim,S]*/,
                         const float* bias /*[dim]*/, int64_t dim, int64_t* species_index, int32_t* species_i32,
                         float* node_feats, float* node_attrs, int32_t* err_flag, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * with_edge_vectors (nn/_nequip.py:214-268) + o3.SphericalHarmonics (nn/_nequip.py:167-174)
 * + soft_one_hot_linspace bessel * sqrt(nb) (nn/embedding.py:185-199), fused, per edge.
 *   vec = pos[dst] - pos[src] + shift . cell[batch[src]]
 * Sorted-order outputs (consumed by the kernels below; e = sorted position, o = perm[e]):
 *   geom_sorted[E,4] = (vx, vy, vz, |v|)
 *   sh_sorted[E, sh_stride]   real SH of v/|v| in the first (lmax+1)^2 columns, l-major, m=-l..l,
 *                             'component' normalised; sh_stride >= (lmax+1)^2 (32 keeps rows on 128-B lines);
 *                             the remaining columns of every row are written as zeros (no pre-clearing needed)
 * Optional original-order outputs for the backbone's data dict (NULL to skip):
 *   edge_vectors[E,3], edge_lengths[E], edge_attrs[E,(lmax+1)^2], edge_embedding[E,nb]
 * cell is [B,3,3] (rows = lattice vectors) or NULL; n_cells==1 uses cell 0 for every edge.
 * Node ids outside [0, n_nodes) and crystal ids outside [0, n_cells) are clamped (memory safety only: matten_csr_build
 * flags such a batch, and the host may read that flag after this kernel was enqueued).
 * ------------------------------------------------------------------------------------------ */
int matten_edge_geom(const float* pos, const int64_t* edge_index, const float* edge_cell_shift,
                     const float* cell, int64_t n_cells, const int64_t* batch, const int32_t* perm,
                     int64_t n_edges, int64_t n_nodes, int lmax, int n_basis, float r_start, float r_end,
                     float* geom_sorted, float* sh_sorted, int sh_stride, float* edge_vectors, float* edge_lengths,
                     float* edge_attrs, float* edge_embedding, matten_stream_t stream);
/* Adjoint of matten_edge_geom w.r.t. positions and cells (the reference differentiates with_edge_vectors,
 * nn/_nequip.py:214-268, and o3.SphericalHarmonics, nn/_nequip.py:167-174, by autograd).  Per sorted edge e, with
 * n = v / max(r, 1e-12) from geom_sorted:
 *   dn   = J(n)^T dy[e, 1:]          J: the polynomial derivative of the harmonics (column 0 contributes nothing)
 *   dv_e = dlen[e] n + (dn - (n . dn) n) / max(r, 1e-12)                   (dv_e = 0 where r < 1e-12)
 * then, in a fixed order and without atomics,
 *   dpos[a]      = sum_{e in [rowptr[a], rowptr[a+1])} dv_e - sum_{t in [out_ptr[a], out_ptr[a+1])} dv_{out_perm[t]}
 *   dcell[b,k,:] = sum over the crystal's sorted edges, ascending, of edge_cell_shift[perm[e], k] dv_e
 * (out_ptr / out_perm: the source-keyed CSR of matten_tp_backward_lit).  A crystal's edges are the contiguous range
 * rowptr[ptr[b]] .. rowptr[ptr[b+1]] (ptr [n_cells+1] int64: first atom of every crystal); with n_cells == 1 the range
 * is every edge and ptr may be NULL.  dy [E, sh_stride] and dlen [E] are the sums over all conv layers; either may be
 * NULL.  dcell may be NULL (then edge_cell_shift, perm, ptr are not read: open structures have no shift term).
 * dv [E,4] is caller-owned scratch.  n_edges == 0 zeroes dpos [n_nodes,3] and dcell [n_cells,3,3].  Nothing synchronises. */
int matten_edge_geom_bwd(const float* geom_sorted, const float* dy, int64_t sh_stride, const float* dlen, int lmax,
                         int64_t n_edges, int64_t n_nodes, const int32_t* rowptr, const int32_t* out_ptr,
                         const int32_t* out_perm, const int32_t* perm, const float* edge_cell_shift, int64_t n_cells,
                         const int64_t* ptr, float* dv, float* dpos, float* dcell, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Radial MLP: e3nn FullyConnectedNet([nb, h, h, W], act=silu) applied to the Bessel embedding
 * (nn/utils.py:246-251,260 <- nn/conv.py:113).  fp32 MFMA (v_mfma_f32_16x16x4_f32).
 *   in : geom_sorted[E,4] (uses |v|); the Bessel basis is recomputed in the prologue
 *   w0p[nb_pad, h], w1p[h, h], w2p[h, w_pad]: weights pre-scaled by 1/sqrt(fan_in) and by the
 *        normalize2mom constant of the *previous* activation, row-major, zero padded
 *        (nb_pad multiple of 4, h == 32, w_pad multiple of 16)
 *   out: w_edge[E, w_pad] fp32, or bf16 (round to nearest even) when out_is_bf16
 * ------------------------------------------------------------------------------------------ */
int matten_radial_mlp(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                      const float* w0p, int nb_pad, const float* w1p, const float* w2p, int hidden, int w_pad,
                      float act_cst, void* w_edge, int out_is_bf16, matten_stream_t stream);
int matten_radial_mlp_deep(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                           const float* w0p, int nb_pad, const float* w_mid, int n_mid, const float* w2p, int hidden,
                           int w_pad, float act_cst, void* w_edge, int out_is_bf16, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 'uvu' TensorProduct + gather + scatter-add + neighbour normalisation over MATERIALISED per-edge weights
 * (nn/utils.py:230-237,263; nn/conv.py:113-120):
 *   agg[n, slot(p,u,k)] = norm_n * sum_{e in in(n)} w[e, woff_p+u] * sqrt(2 l3+1) sum_ij C^{l1 l2 l3}_{ijk} x[src_e, xoff_p+u*d1+i] Y_{l2,j}(e)
 *   norm_n = 1/sqrt(avg_num_neighbors) if avg_num_neighbors > 0 else 1/sqrt(num_neigh[n])
 * One wave per (path, node group), a lane owns one output channel of one destination node, CG coefficients are
 * compile-time literals (l <= 4).  The training forward (its adjoint reads the same w), and an independent implementation
 * of the contraction the production kernel matten_tp_fused is tested against.
 *   path_entries[n_entries, 8] int32 {l1*25+l2*5+l3, x_off, w_off, out_off, mul(<=64), log2(lanes per node), 0, 0}
 *   unit_start[n_entries+1]   int32  prefix sum of waves per node tile (matten_tp_tile_nodes() nodes per tile)
 * ------------------------------------------------------------------------------------------ */
int matten_tp_tile_nodes(void);
/* (w_edge: fp32, or bf16 when w_is_bf16 -- the opt-in bf16 storage of the training step's per-edge tensors) */
int matten_tp_paths(const float* x, int64_t d_in, const void* w_edge, int64_t w_pad, const float* sh_sorted,
                    int64_t sh_dim, const int32_t* rowptr, const int32_t* src_sorted, int64_t n_nodes,
                    const int32_t* path_entries, const int32_t* unit_start, int64_t n_entries,
                    int64_t units_per_tile, int64_t d_mid, float avg_num_neighbors, const float* num_neigh,
                    float* agg /*[N,d_mid]*/, int w_is_bf16, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * lin2 of a conv layer as a row stream over COMPONENT-MAJOR neighbour sums (reference nn/conv.py:84-86,123:
 * out = FullyConnectedTensorProduct(agg, one_hot(species)) + self-connection).
 *   agg[N, ld]: per output irrep io of lin2 a region [component k][channel slot 0..16 T_io): the channels of every
 *               path with that irrep side by side (written by matten_tp_fused when group_entries word 8+c (t_off[c])
 *               holds the component stride 16 T_io and word 20+c (out_off[c]) the first float of the entry's channel 0);
 *               regions back to back, so chunk f (16 floats) of a row belongs to exactly one (io, k)
 *   io_table[n_io, 8] int32: {first chunk, T, K (channel slots used; the rest are never read as data),
 *               d3 | n_mt << 8 | cw << 16, a_off, out_off, mul_out, 0}
 *   blocks[n_blocks, 4] int32: the row cut into runs of <= 8 chunks of one (io, k), front to back:
 *               {first chunk, n | first-of-unit << 8 | last-of-unit << 9 | last unit of the table row << 10 | k << 12 |
 *               io << 20, chunk index inside the unit, 0}; a table row has mul_out * d3 <= 32 (wider irreps: several rows)
 *   wtab[n_species, w_stride]: per species and irrep the weights as MFMA A fragments at a_off,
 *               [t < T][mt < n_mt][g < 4][c < cw][s < 4] = fan^-1/2 W_s[slot 16 t + 4 g + s][v = 16 mt + c] (cw = 16 or mul_out)
 *   order / seg: rows sorted by species + per-species offsets (matten_group_by_key), or NULL/NULL with n_species == 1
 *   out[N, d_out] in the reference's mul_ir layout: out[n, out_off + v d3 + k] = add[...] + sum
 * ------------------------------------------------------------------------------------------ */
int matten_agg_linear_max_mt(void);        /* column tiles per io_table row (mul_out of a row <= 16 * this) */
int matten_agg_linear_block_chunks(void);  /* chunks per block (the n of a blocks[] row is <= this) */
size_t matten_agg_linear_lds_bytes(int64_t w_stride, int64_t n_io, int64_t n_blocks);   /* LDS a launch needs ... */
size_t matten_agg_linear_max_lds_bytes(void);                                          /* ... and may have */
int matten_agg_linear(const float* agg, int64_t ld, const int32_t* order, const int32_t* seg, int64_t n_species,
                      const float* wtab, int64_t w_stride, const int32_t* io_table, int64_t n_io,
                      const int32_t* blocks, int64_t n_blocks, const float* add, int64_t add_ld, int64_t d_out,
                      int64_t n_rows, float* out, matten_stream_t stream);
/* matten_agg_linear with the conv layer's Gate (reference nn/utils.py:134-140) and eval-mode BatchNorm (:418,432)
 * applied in the epilogue: out [n_rows, d_act] is the ACTIVATED row, the conv output row [n_rows, d_out] never exists.
 *   cmeta[d_out, 4] int32 per column of lin2's output {type | act << 8, column in the activated row, gate lane, gate set}:
 *     type 1 activated scalar, 2 gate scalar (kept in registers: set < matten_agg_linear_gate_sets(), lane = its position
 *     in the table row that produced it), 3 gated component; gates are produced by table rows that precede their users
 *     (host: plan.plan_agg_gate);  act codes and act_cst[8] as matten_gate_bn;
 *   bn_scale / bn_shift [d_act] (both or NULL): weight / sqrt(running_var + eps) and, on 0e columns,
 *     bias - running_mean * scale */
int matten_agg_linear_gate(const float* agg, int64_t ld, const int32_t* order, const int32_t* seg, int64_t n_species,
                           const float* wtab, int64_t w_stride, const int32_t* io_table, int64_t n_io,
                           const int32_t* blocks, int64_t n_blocks, const float* add, int64_t add_ld, int64_t d_out,
                           int64_t n_rows, const int32_t* cmeta, const float* act_cst, const float* bn_scale,
                           const float* bn_shift, int64_t d_act, float* out, matten_stream_t stream);
int matten_agg_linear_gate_sets(void);
/* ------------------------------------------------------------------------------------------
 * Fused production path of one conv layer's edge work (reference nn/utils.py:246-251,260,263 +
 * nn/conv.py:113-120): the per-edge radial weights are never written to memory.
 *   matten_radial_hidden: rbf(|v|) -> 32 -> 32 (silu), fp32 MFMA; writes h2s[E,2,32] fp16 (128 B per edge): every
 *                         hidden feature v as two pieces, v = hi + 2^-11 lo (hi = fp16(v), lo = fp16(2^11 (v - hi)),
 *                         fp16 subnormals zeroed: v to 2^-24 relative); column g*8+kk of piece 0 (hi) / piece 1 (lo)
 *                         holds hidden feature 16*(kk>>2) + 4*g + (kk&3)
 *   matten_tp_fused:      per (input block, l2 group, node group) wave: last MLP layer on the matrix
 *                         cores (w = h2 . W2p as three fp16 products hi.hi + 2^-11 (hi.lo + lo.hi) accumulated in
 *                         fp32: fp32-class rounding at 1/5 of the fp32 MFMA time) into a wave-private LDS tile, consumed in place by the
 *                         literal-coefficient CG contraction + CSR neighbour sum
 *   w2p[32, w_pad]: last layer weights pre-scaled (1/sqrt(32) * normalize2mom(silu)), columns in the
 *                   fused [entry][u][coupling] order of group_entries, w_pad >= w_cols + 16, the columns from w_cols on ZERO
 *                   (whole tiles are read from any entry on; the stage rows of an empty segment are read from the last four)
 *   group_entries[n_entries, 32] int32 {l1*8+g, x_off, mul, log2(lanes per node), coupling mask, w_base, first A tile,
 *                   A tiles, t_off[12], out_off[12]}: one entry per (input irrep block chunk, l2 group g); couplings in the
 *                   order of cg_gen.h Group<l1,g>, weight columns [u][c] (absent couplings: zero columns), mul * couplings
 *                   <= matten_tp_max_cols*(); word 0 + 256: a merged entry (two two-channel blocks, its second record
 *                   follows); word 0 + 512: weight columns coupling-major, column mul * c + u, for an entry with mul == lanes
 *                   per node == 16 or 8 and l1 < matten_tp_wreg(): shared and paired workgroups pass its weights from the
 *                   matrix phase to the contraction in registers instead of through the LDS tile; out_off[c] = first float of channel 0 in the output row, t_off[c] = 0
 *                   (the reference's mul_ir row) or the floats between two components (component-major row)
 *   unit_map[units_per_tile]: wave index inside a node tile -> flags | entry << 8 | node group (of 64 >> cu_log2 nodes);
 *                   flags: bit 24 = the unit's workgroup (four consecutive units) shares an LDS stage: same node
 *                   group and lanes per node -- or, with bit 26 (paired), units 0,1 on node group r and units 2,3 the
 *                   same two entries on r + 1; bit 25 = loader-only unit (feeds the stage, contracts nothing).  Any
 *                   bijection is valid, the host orders it node group first (plan.fused_unit_map) so the waves of a
 *                   workgroup read the same hidden-feature / harmonics rows
 *   a_split / a_scale_inv (both or neither; NULL: the kernel splits w2p itself, ~400 instructions per wave):
 *                   w2p as ready-made MFMA A fragments.  Entry e owns tiles [a_tile, a_tile + n_mt) (group_entries
 *                   words 6, 7); tile t, lane (g = lane >> 4, c = lane & 15) holds 16 fp16: hi[kk], lo[kk], kk < 8, of
 *                   s_e * w2p[16 (kk >> 2) + 4 g + (kk & 3)][w_base + 16 (t - a_tile) + c] with s_e the power of two
 *                   that puts the entry's largest magnitude in [2^13, 2^14); a_scale_inv[e] = 1 / (s_e h_scale)
 *   lds_floats_per_wave: max over entries of 16*T*(16*ceil(mul*NC/16)+36), T = max(1, nodes_per_wave/16)
 *                   (sh_sorted rows must be 32 floats apart: sh_stride == 32)
 *   h_scale (device pointer to ONE float, or NULL = 1): power of two the hidden features are multiplied by before
 *                   the fp16 split, chosen by the host so that |h_scale * h2| < 2^15 for ANY edge (from the weights'
 *                   column sums: 1 for a normally scaled MLP); the caller multiplies a_scale_inv by 1 / h_scale
 */
int matten_radial_hidden(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                         const float* w0p, int nb_pad, const float* w1p, int hidden, uint16_t* h2s,
                         const float* h_scale, matten_stream_t stream);
/* the same for n_layers <= 8 radial MLPs over one edge list in ONE launch (every conv layer of a model reads the same
 * edge lengths; the Bessel basis is evaluated once): w0p / w1p / h2s / h_scale (or NULL) are HOST arrays of n_layers
 * device pointers */
int matten_radial_hidden_multi(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                               const float* const* w0p, int nb_pad, const float* const* w1p, int hidden,
                               uint16_t* const* h2s, const float* const* h_scale, int n_layers,
                               matten_stream_t stream);
/* any depth: h2s holds the LAST hidden layer's features (same form); w_mid of the multi launch is a host array of
 * n_layers device pointers, every MLP with the same n_mid */
int matten_radial_hidden_deep(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                              const float* w0p, int nb_pad, const float* w_mid, int n_mid, int hidden, uint16_t* h2s,
                              const float* h_scale, matten_stream_t stream);
int matten_radial_hidden_multi_deep(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                                    const float* const* w0p, int nb_pad, const float* const* w_mid, int n_mid, int hidden,
                                    uint16_t* const* h2s, const float* const* h_scale, int n_layers,
                                    matten_stream_t stream);
int matten_tp_fused(const float* x, int64_t d_in, const uint16_t* h2s, const float* w2p, int64_t w_pad,
                    const float* sh_sorted, int64_t sh_stride, const int32_t* rowptr, const int32_t* src_sorted,
                    int64_t n_nodes, const int32_t* group_entries, const int32_t* unit_map, int64_t n_entries,
                    int64_t units_per_tile, int64_t lds_floats_per_wave, int64_t d_mid, float avg_num_neighbors,
                    const float* num_neigh, const uint16_t* a_split, const float* a_scale_inv,
                    float* agg /*[N,d_mid]*/, matten_stream_t stream);
/* matten_tp_fused for the entries of plan.plan_agg_narrow (word 0 + 1024: the entry has narrowed couplings).  lin2 maps the mul
 * channels of a coupling onto the mo channels of its output irrep; where mo < mul the entry's lanes apply their own slice of
 * lin2 to their sums -- partial[v][k] = sum_u W[species][u][v] * sum[u][k], added over the node's lanes in a fixed order
 * -- and store mo floats per component at out_off[c] + k * t_off[c] instead of mul (matten_agg_linear then reads them with
 * the A value 1).  Narrowed entries have mul == lanes per node == 8 or 16, l1 <= matten_tp_narrow_max_l1(), the coupling-major
 * flag (+ 512) and mo in {1, 2, 4}; every other coupling is written as by matten_tp_fused.
 *   group_entries: ONE buffer [entries n_entries x 32 | weights] (plan.narrow_blob): the kernel has no scalar registers for
 *                  further pointers and finds the weights from the entry record.  The two words of a narrowed coupling c:
 *                  t_off[c] = floats between components | mo << 20, out_off[c] = first float (< 65536) | distance of the
 *                  coupling's weight block [species][u < mul][v < mo] (fp32, lin2's fan-in normalisation included) from the
 *                  ENTRY in units of four floats << 16; mo == 0: a plain coupling
 *   species[n_nodes] int32: species index per destination node (required; all 0 for one species)
 *   d_mid a multiple of 4, out_off[c] of a narrowed coupling a multiple of its mo (pieces of 4 mo bytes) */
int matten_tp_fused_narrow(const float* x, int64_t d_in, const uint16_t* h2s, const float* w2p, int64_t w_pad,
                           const float* sh_sorted, int64_t sh_stride, const int32_t* rowptr, const int32_t* src_sorted,
                           int64_t n_nodes, const int32_t* group_entries, const int32_t* unit_map, int64_t n_entries,
                           int64_t units_per_tile, int64_t lds_floats_per_wave, int64_t d_mid, float avg_num_neighbors,
                           const float* num_neigh, const uint16_t* a_split, const float* a_scale_inv,
                           const int32_t* species, float* agg /*[N,d_mid]*/, matten_stream_t stream);
int matten_tp_narrow_max_l1(void);   /* largest l1 of an input block whose entries may carry narrowed couplings */

int matten_tp_wreg(void);       /* 0: no entry may carry the coupling-major flag (built with -DTPF_WREG=0); else 1 + the largest l1 that may */
int matten_tp_max_cols(void);   /* weight columns (mul * couplings) a group entry of matten_tp_fused may have */
int matten_tp_max_cols_l0(void);   /* the same for entries of scalar (l1 = 0) input blocks */
int matten_tp_max_cols_l1(void);   /* ... and of vector (l1 = 1) input blocks */
/* 31-bit hash of the coupling-group lists the library's generated coupling code (csrc/cg_gen.h) was built for; the host plans
 * entries for the lists of matten_amd/plan.py (plan.tp_groups_hash) and refuses a library built for others. */
int matten_tp_groups_hash(void);

/* ------------------------------------------------------------------------------------------
 * FullyConnectedTensorProduct(x, one_hot(species)) == species-indexed per-irrep linear
 * (nn/conv.py:59-61,77-79,84-86 called :109,112,123), and e3nn o3.Linear when species == NULL
 * (nn/nodewise.py:111-117, model_factory/tfn_scalar_tensor.py:49-51,68).
 *   out[n, o_off + w*d + k] = (add ? add[..] : 0) + sum_{u<mul_in} Wp[species(n), w_off + u*mo + w] * x[n, x_off + u*d + k]
 *   x rows are d_in floats apart, out rows d_out, add rows add_ld (>= d_out; a column slice of a wider matrix is fine:
 *   the conv layer evaluates lin1 and the self-connection as one call and hands the second half on as the addend)
 *   for every segment, w < mo, k < d.  fp32 MFMA over tiles of 16 rows x 16 output channels.
 *   segs[n_segs, 8] int32 {x_off, d, mul_in, w_off, mo, o_off, 0, 0}: one per (input irrep block ->
 *       output irrep block) path; outputs no segment covers are NOT written (the caller zero-fills
 *       unreachable irreps)
 *   Wp[n_species, w_stride]: weights repacked per species with the path normalisation folded in.
 *   order[N] / seg[n_species+1]: node ids sorted by species and the offsets of each species' run
 *   (e.g. perm / rowptr of matten_csr_build over {row0 = node id, row1 = species}); both NULL for a
 *   plain linear (n_species == 1).  Rows are processed species by species so the weight table of
 *   one species is staged on chip once per workgroup; outputs land at their original row.
 * ------------------------------------------------------------------------------------------ */
int matten_species_linear(const float* x, int64_t d_in, const int32_t* order, const int32_t* seg, int64_t n_species,
                          const float* wp, int64_t w_stride, const int32_t* segs, int64_t n_segs, int64_t d_out,
                          const float* add, int64_t add_ld, int64_t n_rows, float* out, matten_stream_t stream);

/* Same operator, same arguments, for SHORT rows (16 * (d_in | 1) + w_stride floats <= 64 KB of LDS, one segment table):
 * a workgroup keeps its 16 rows and the species' weights in LDS and walks the irrep blocks without the streaming
 * kernel's chunk pipeline (reference call sites nn/conv.py:109,112 lin1 / self-connection, nn/nodewise.py:116).
 * Returns MATTEN_EINVAL when the rows do not fit: call matten_species_linear then. */
int matten_species_linear_rows(const float* x, int64_t d_in, const int32_t* order, const int32_t* seg, int64_t n_species,
                               const float* wp, int64_t w_stride, const int32_t* segs, int64_t n_segs, int64_t d_out,
                               const float* add, int64_t add_ld, int64_t n_rows, float* out, matten_stream_t stream);

/* The launchers' own thresholds (the constants they branch on), for routing checks on the host: */
int matten_species_linear_walk_all_blocks(void);      /* cdiv(n_rows, 64) + n_species (0 for a plain linear) from which ONE
                                                         workgroup walks all irrep blocks; below it one block per blockIdx.y */
int64_t matten_species_linear_lds_w_floats(void);     /* largest w_stride (rounded up to 4) whose table is kept in LDS; above
                                                         it the A operand is read from global memory */
int64_t matten_species_linear_rows_lds_bytes(void);   /* matten_species_linear_rows refuses layouts above this many bytes:
                                                         4 * (16 * (d_in | 1) + round4(w_stride) + 8 * n_segs) */

/* ------------------------------------------------------------------------------------------
 * e3nn Gate (nn/utils.py:134-140,158-159 <- nn/conv.py:209) fused with e3nn BatchNorm in eval
 * mode (nn/utils.py:418,432-433 <- nn/conv.py:211).
 *   meta[d_out] int4 {src, gate(-1: scalar), act (0 none,1 silu,2 tanh,3 sigmoid,4 ssp,5 abs) | gate_act<<8, bn_idx | mean_idx<<16 (0xFFFF: none)}
 *   out = act(x[src])*c_act                      (scalars)
 *       = x[src] * gate_act(x[gate])*c_gate      (gated irreps)
 *   then, if bn_weight != NULL: (out - running_mean[mean_idx]) * rsqrt(running_var[bn_idx]+eps)*bn_weight[bn_idx] + bn_bias[mean_idx]
 *   act_cst[8]: normalize2mom constants indexed by act code.
 * ------------------------------------------------------------------------------------------ */
int matten_gate_bn(const float* x, int64_t d_in, const int32_t* meta, int64_t d_out, const float* act_cst,
                   const float* running_mean, const float* running_var, const float* bn_weight,
                   const float* bn_bias, float eps, int64_t n_rows, float* out, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * NodewiseReduce: torch_scatter.scatter(x, batch, reduce=mean|sum) over contiguous crystals
 * (nn/nodewise.py:142-148).  ptr[B+1] int64 (PyG convention).  mean divides by max(count,1).
 * ------------------------------------------------------------------------------------------ */
int matten_segment_reduce(const float* x, int64_t dim, const int64_t* ptr, int64_t n_segments, int mean,
                          float* out, matten_stream_t stream);
/* reduce = min | max (the other two values nn/nodewise.py:131 accepts): per crystal and column the smallest / largest
 * value and, in arg [n_segments, dim] int64 (optional), the row it came from (an empty crystal: 0 and -1);
 * _bwd: dx[arg[b, c], c] = dy[b, c], dx zero-initialised */
int matten_segment_minmax(const float* x, int64_t dim, const int64_t* ptr, int64_t n_segments, int take_max, float* out,
                          int64_t* arg, matten_stream_t stream);
int matten_segment_minmax_bwd(const float* dy, int64_t dim, const int64_t* arg, int64_t n_segments, float* dx,
                              matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Adjoint of the radial MLP (training; reference nn/utils.py:246-251,260 differentiated by autograd there).
 * Inputs as matten_radial_mlp (packed weights; w2p in the column order of dw), plus dw[E, dw_ld] = dL/dw from
 * matten_tp_backward (fp32, or bf16 when dw_is_bf16; only the first w_cols columns are read as data).
 * Outputs are PARTIAL sums the caller adds up (fixed order, no atomics):
 *   part_small[matten_radial_mlp_bwd_small_slices(E)][nb_pad*32 + 32*32]: scale0 d/dW0p [nb_pad,32], scale1 d/dW1p [32,32]
 *   part_w2[matten_radial_mlp_bwd_w2_ranges(E, w_pad)][32][w_pad]:        scale2 d/dW2p
 *   h2_scratch[E, 32]: workspace (the recomputed hidden features, written by the first kernel, read by the second)
 * ------------------------------------------------------------------------------------------ */
int64_t matten_radial_mlp_bwd_small_slices(int64_t n_edges);
int64_t matten_radial_mlp_bwd_w2_ranges(int64_t n_edges, int64_t w_pad);
int matten_radial_mlp_bwd(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                          const float* w0p, int nb_pad, const float* w1p, const float* w2p, int hidden, int w_pad,
                          int w_cols, const void* dw, int64_t dw_ld, int dw_is_bf16, float* h2_scratch,
                          float* part_small, float* part_w2, float scale0, float scale1, float scale2,
                          float* grad_small, float* grad_w2, matten_stream_t stream);
/* grad_small [nb_pad*32 + 32*32] / grad_w2 [32, w_pad] (both or neither, may be NULL): the partial sums added up in slice
 * order by a third launch of the same call.
 * _deep: a slice of part_small / grad_small is [nb_pad*32 + n_mid*32*32]: scale0 d/dW0p, then scale1 d/dWmid_p[i] for
 * i = 0 .. n_mid-1; h2_scratch holds the last hidden layer.  The slice count does not depend on n_mid, the range
 * count does: part_w2 has matten_radial_mlp_bwd_w2_ranges_deep(E, w_pad, n_mid) rows. */
int64_t matten_radial_mlp_bwd_w2_ranges_deep(int64_t n_edges, int64_t w_pad, int n_mid);
int matten_radial_mlp_bwd_deep(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                               const float* w0p, int nb_pad, const float* w_mid, int n_mid, const float* w2p, int hidden,
                               int w_pad, int w_cols, const void* dw, int64_t dw_ld, int dw_is_bf16, float* h2_scratch,
                               float* part_small, float* part_w2, float scale0, float scale1, float scale2,
                               float* grad_small, float* grad_w2, matten_stream_t stream);
/* Adjoint of the radial MLP w.r.t. its INPUT, the edge length (the reference differentiates soft_one_hot_linspace,
 * nn/embedding.py:185-199, and FullyConnectedNet, nn/utils.py:246-251,260, by autograd).  One entry for every depth:
 * w_mid [n_mid,32,32], n_mid = 0 .. 3 (NULL at 0); the packed layers as matten_radial_mlp_deep takes them; dw as above.
 *   dlen[e] = sum_k dL/demb[e,k] b_k'(r_e),   b_k(r) = sqrt(2/c) sqrt(nb) sin((k+1) pi x / c) / x,  x = r - r_start,
 *   c = r_end - r_start;  b_k' = 0 where b_k is (x <= 0 or x >= c)
 * dL/demb comes from dw back through the last layer (the same dw W2p^T stage on the matrix cores as the weight
 * adjoint), the silu layers (recomputed from r) and the first layer.  dlen [E] fp32, every element written. */
int matten_radial_mlp_bwd_len(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                              const float* w0p, int nb_pad, const float* w_mid, int n_mid, const float* w2p, int hidden,
                              int w_pad, int w_cols, const void* dw, int64_t dw_ld, int dw_is_bf16, float* dlen,
                              matten_stream_t stream);
/* the raw layers (w0 [nb,32], w1 [32,32], w2 [32,W]) -> packed operands w0p = scale0 w0 (rows padded to nb_pad),
 * w1p = scale1 w1, w2p = scale2 w2 (columns padded to w_pad), one launch; matten_radial_mlp_bwd multiplies its partial
 * sums by the same three factors, so they are gradients w.r.t. the RAW layers */
int matten_radial_pack(const float* w0, const float* w1, const float* w2, int n_basis, int nb_pad, int w_cols, int w_pad,
                       float scale0, float scale1, float scale2, float* w0p, float* w1p, float* w2p,
                       matten_stream_t stream);
/* _deep: w_mid [n_mid,32,32] raw -> w_mid_p = scale1 w_mid (the same factor for every middle layer) */
int matten_radial_pack_deep(const float* w0, const float* w_mid, int n_mid, const float* w2, int n_basis, int nb_pad,
                            int w_cols, int w_pad, float scale0, float scale1, float scale2, float* w0p, float* w_mid_p,
                            float* w2p, matten_stream_t stream);
/* Operands of matten_tp_fused derived from the RAW radial layers by kernels (training on the production kernel):
 * matten_radial_pack_cols: as matten_radial_pack, the last layer gathered through cols[n_cols] int64 (fused column order
 *   of plan.fused_cols, -1 = zero column), zero up to w_pad;
 * matten_radial_h_scale: out2 = [s, 1/s], the power of two <= 1 that keeps the hidden features inside the fp16 range
 *   (bound from the hidden layers' column-sum norms, as nn/utils.py RadialMLP._fp16_scale: P(c) n0 n_1 ... n_{n_mid});
 * matten_split_a_tiles: w2p [32, w_pad] -> the fp16 hi / lo A fragments of every group entry (word 5 = first column,
 *   6 = first tile, 7 = tile count) + scale_inv[n_entries] = 1 / (entry scale) * h_scale[1] (h_scale may be NULL). */
int matten_radial_pack_cols(const float* w0, const float* w1, const float* w2, int n_basis, int nb_pad, int w_cols,
                            const int64_t* cols, int n_cols, int w_pad, float scale0, float scale1, float scale2, float* w0p,
                            float* w1p, float* w2p, matten_stream_t stream);
int matten_radial_h_scale(const float* w0, const float* w1, int n_basis, float r_start, float r_end, float act_cst,
                          float* out2, matten_stream_t stream);
int matten_radial_pack_cols_deep(const float* w0, const float* w_mid, int n_mid, const float* w2, int n_basis, int nb_pad,
                                 int w_cols, const int64_t* cols, int n_cols, int w_pad, float scale0, float scale1,
                                 float scale2, float* w0p, float* w_mid_p, float* w2p, matten_stream_t stream);
int matten_radial_h_scale_deep(const float* w0, const float* w_mid, int n_mid, int n_basis, float r_start, float r_end,
                               float act_cst, float* out2, matten_stream_t stream);
int matten_split_a_tiles(const float* w2p, int64_t w_pad, const int32_t* group_entries, int64_t n_entries,
                         const float* h_scale, uint16_t* frag, float* scale_inv, matten_stream_t stream);
/* out[i] = src[idx[i]] * scale[(scale_by_source ? idx[i] : i) % scale_period]: the per-species re-packing of a flat e3nn
 * weight (idx = gather table, scale by output position) and its adjoint (idx = inverse permutation, scale by source) */
int matten_gather_scale(const float* src, const int64_t* idx, const float* scale, int64_t n, int64_t scale_period,
                        int scale_by_source, float* out, const int64_t* perm2, float* out2, matten_stream_t stream);
/* perm2 [scale_period] / out2 (both or neither): a second output with the columns of every period permuted,
 * out2[r, q] = out[r, perm2[q]] -- the transposed packed weights of the species linear's adjoint in the same launch */
int64_t matten_species_linear_wgrad_scratch_floats(int64_t n_rows, int64_t n_species, int64_t w_stride);   /* matten_species_linear_wgrad's scratch */

/* ------------------------------------------------------------------------------------------
 * CartesianTensor.to_cartesian (utils.py:123-124, predict.py:145): out[b,:] = x[b,:] @ Q
 *   Q [n_in, n_out] row-major (n_in = 21, n_out = 81 for ijkl=jikl=klij)
 * ------------------------------------------------------------------------------------------ */
int matten_dense_rows(const float* x, int64_t n_in, const float* q, int64_t n_out, int64_t n_rows, float* out,
                      matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Derived elastic properties (predict.py:217-218: `predictions = [ElasticTensor(t) for t in predictions]` -- what the
 * reference's users read off pymatgen's ElasticTensor, one Python object per crystal there).  fp64 arithmetic.
 * Voigt order xx, yy, zz, yz, xz, xy; C_IJ = C_ijkl without factors, S = inverse of that 6x6 matrix (engineering
 * convention: the factors 2 and 4 live in S).  Values are in the units of the input (pymatgen's y_mod alone is
 * multiplied by 1e9; not here).
 * matten_elastic_props: one crystal per thread.
 *   c: fp32 (is_fp64 = 0) or fp64 (1); layout 0 = Cartesian [n,81] (= [n,3,3,3,3]), 1 = Voigt [n,36].  The input is
 *   symmetrised first: the mean of the 8 Cartesian entries equivalent under ij<->ji, kl<->lk, (ij)<->(kl), or (C + C^T)/2.
 *   voigt [n,36], compliance [n,36] (Gauss-Jordan with partial pivoting: indefinite tensors are inverted too),
 *   props [n,10] = k_voigt, g_voigt, k_reuss, g_reuss, k_vrh, g_vrh, y_mod (9KG/(3K+G) of the VRH means),
 *   homogeneous_poisson, universal_anisotropy (5 g_voigt/g_reuss + k_voigt/k_reuss - 6), pugh_ratio (k_vrh/g_vrh);
 *   flags [n] int32: bit 0 = singular or non-finite input, every output of the row is NaN; bit 1 = not positive definite
 *   (un-pivoted LDL^T; the values are still computed; also set on every row with bit 0).
 * matten_elastic_props_bwd: the adjoint of matten_elastic_props, one crystal per thread, from what the forward wrote.
 *   voigt, compliance [n,36], props [n,10], flags [n]: as matten_elastic_props returned them.  g_props [n,10], g_voigt
 *   [n,36], g_compliance [n,36] (fp64): the upstream gradients; g_voigt and g_compliance may each be NULL (= zero).
 *   g_c [n,81] (layout 0) or [n,36] (layout 1), fp32 (is_fp64 = 0) or fp64 (1): the gradient of the forward's input c, every
 *   element written.  The scalars' gradients are folded into the Voigt and Reuss bounds, those onto the entries of C and S
 *   that the forward summed; the inverse gives Cbar -= S^T Sbar S^T (Sbar a general 6x6); last the transpose of the
 *   symmetrisation (layout 0: the 8-position mean, coinciding positions counted twice; layout 1: (Cbar + Cbar^T)/2).
 *   A row with flag bit 0 gets zeros whatever the upstream gradients hold (NaN included); a row with bit 1 alone is
 *   differentiated like any other.  No atomics, no cross-thread traffic: bitwise reproducible.
 * matten_elastic_directional: one workgroup per crystal over unit directions dirs [n_dirs,3] (fp64, n_dirs >= 1).  With
 *   v(n) = (n1^2, n2^2, n3^2, n2 n3, n1 n3, n1 n2): Young's modulus E(n) = 1 / (v^T S v), linear compressibility
 *   beta(n) = sum_I (S_I1 + S_I2 + S_I3) v_I, S = the mean of the two triangles of compliance [n,36].
 *   young / beta [n,n_dirs]: optional, NULL = not written.  ext [n,4] = E_min, E_max, beta_min, beta_max; arg [n,4] int32 =
 *   their direction indices, equal values resolved to the lowest index (bitwise reproducible).  Rows with flag bit 0: NaN
 *   and -1.
 * matten_elastic_pair (predict.py:217-218: what pymatgen's users compute one pair at a time from the compliance tensor):
 *   shear modulus and Poisson's ratio over pairs of perpendicular unit directions, one workgroup per crystal, a lane per
 *   direction n, the lane looping over the n_angles directions m_k = cos(chi_k) e1 + sin(chi_k) e2 perpendicular to it.
 *   cos_sin [n_angles,2] fp64 = (cos chi_k, sin chi_k), made by the host (chi_k = pi k / n_angles: m and -m count once);
 *   (e1, e2) the branch-free orthonormal frame of n: s = n3 >= 0 ? 1 : -1, a = -1/(s + n3), b = n1 n2 a,
 *   e1 = (1 + s n1^2 a, s b, -s n1), e2 = (b, s + n2^2 a, -n2).  With v() as above and
 *   w(n,m) = (2 n1 m1, 2 n2 m2, 2 n3 m3, n2 m3 + n3 m2, n1 m3 + n3 m1, n1 m2 + n2 m1):
 *   1/G(n,m) = w^T S w,  nu(n,m) = -(v(n)^T S v(m)) / (v(n)^T S v(n)).
 *   ext [n,4] = G_min, G_max, nu_min, nu_max over all pairs; arg [n,4] int32 = their flat pair index d n_angles + k
 *   (n_dirs n_angles <= 2^31 - 1), equal values resolved to the lowest index; maps [n,n_dirs,4]: optional, the same four
 *   extremes over chi per direction.  Rows with flag bit 0: NaN and -1.
 * matten_elastic_acoustic (predict.py:217-218: pymatgen's trans_v / long_v / debye_temperature take VRH averages; this is
 *   the Christoffel equation per direction): Gamma_ik = C_ijkl n_j n_l from voigt [n,36] (the mean of its two triangles),
 *   eigenvalues by cyclic Jacobi in registers, v_i = sqrt(lambda_i modulus_unit / density) ascending (m/s for density in
 *   kg/m^3 and modulus_unit in Pa per unit of C).  A direction with an eigenvalue that is not positive and finite has three
 *   NaN velocities and is counted in n_unstable [n].  vel [n,n_dirs,3]: optional.  ext [n,3] = v_slow_min (the lowest
 *   branch's minimum over the directions), v_fast_max, sum_d sum_i v_i^-3 (lane-strided partial sums, xor butterfly, waves
 *   in index order: bitwise reproducible; NaN with any unstable direction); arg [n,2] int32 = the direction indices of the
 *   two extremes (NaN ignored; -1 if no finite value).  Rows with flag bit 0 or a density that is not positive and finite:
 *   NaN and -1 (n_unstable too).
 * matten_elastic_directional_bwd: the adjoint of matten_elastic_directional, the same launch shape.  compliance, flags, dirs
 *   as the forward took them (nothing else is kept: E(n) is made again).  g_young, g_beta [n,n_dirs]: the maps' upstream
 *   gradients; g_ext [n,4]: those of E_min, E_max, beta_min, beta_max, each sent to the direction arg [n,4] recorded by the
 *   forward (a subgradient where values tie; an index outside 0..n_dirs-1, the forward's -1 included, adds nothing).  Each
 *   of g_young, g_beta, g_ext may be NULL (= zero); g_ext needs arg.  g_compliance [n,36], every entry written:
 *   (H + H^T)/2 with H = sum_d (-gE_d E_d^2 v_d v_d^T + gbeta_d v_d e^T), e = (1,1,1,0,0,0).  Rows with flag bit 0: zeros.
 * matten_elastic_acoustic_bwd: the adjoint of matten_elastic_acoustic, the same launch shape.  The cyclic Jacobi is run again
 *   with the rotations accumulated into eigenvectors u_k; with s = modulus_unit / density and v_k = sqrt(lambda_k s),
 *   w_k = (g_vel_k + [d = arg_0, k = 0] g_ext_0 + [d = arg_1, k = 2] g_ext_1 - 3 g_ext_2 v_k^-4) s / (2 v_k),
 *   Gbar = sum_k w_k u_k u_k^T, Hc[V(i,j)][V(k,l)] += Gbar_ik n_j n_l over the directions, g_voigt [n,36] = (Hc + Hc^T)/2,
 *   every entry written.  g_vel [n,n_dirs,3] and g_ext [n,3] (v_slow_min, v_fast_max, sum of v^-3) may each be NULL (= zero);
 *   g_ext needs arg [n,2].  Rows with flag bit 0 or a density that is not positive and finite: zeros; a direction the
 *   forward marked unstable contributes nothing.  Exactly degenerate modes: per-mode gradients (g_vel, the extremes) take
 *   the orthonormal basis Jacobi left (finite; the derivative is undefined there), the sum's gradient does not depend on it.
 *   Both adjoints: excluded rows and directions are replaced by selects, so a NaN in an upstream gradient there does not
 *   reach the output; lane-strided partial sums, xor butterfly, waves in index order, no atomics: bitwise reproducible.
 * matten_elastic_refine (predict.py:217-218: the extremes pymatgen's users read are as good as their grid; ELATE polishes its
 *   grid's winners in the same way): the extremes of matten_elastic_directional and matten_elastic_pair refined off the grid,
 *   one thread per item = q n + b (extreme-major), q = 0..3 E_min, E_max, beta_min, beta_max from ext_dir / arg_dir [n,4],
 *   q = 4..7 G_min, G_max, nu_min, nu_max from ext_pair / arg_pair [n,4] (only with n_angles >= 1; n_angles = 0: four
 *   extremes, cos_sin / ext_pair / arg_pair are not read and may be NULL).  dirs [n_dirs,3] and cos_sin [n_angles,2] are the
 *   tables the two kernels took; the start pair is n = dirs[d], m = cos(chi_k) e1 + sin(chi_k) e2 in the frame above (k = 0
 *   for E and beta).  E, G, nu: F(w) = +-f(R(w) n, R(w) m), R(w) the rotation by |w| about w, is maximised by a damped Newton
 *   iteration: the gradient at w = 0 is n x dF/dn + m x dF/dm (analytic), the Hessian the symmetric part of that gradient's
 *   central differences over rotations by +-2^-14 rad about the three axes, diagonalised by cyclic Jacobi; every eigenvalue
 *   is clamped to min(lambda, -1e-3 max|lambda|), the step capped at 0.3 rad and accepted only if the value strictly
 *   improves, else damped (doubling, from 1e-3 max|lambda|, 30 tries) and tried again; (n, m) are made orthonormal again
 *   after every step.  It stops when |gradient| <= tol |f| (nu: tol max(|f|, 1)), after max_iter accepted steps, or when no
 *   damped step improves the value any more (stationary to fp64: converged if |gradient| <= max(tol, 1e-7) |f|).
 *   beta(n) = n^T B n, B_ij = sum_k S_ijkk: the extreme eigenvalues of B with their eigenvectors (cyclic Jacobi), no
 *   iteration.  A result that rounding left behind the grid's value gives way to the grid's value and pair.
 *   Outputs, all extreme-major with Q = 4 or 8: value [Q,n]; vec_n, vec_m [Q,n,3] unit and perpendicular (m of E and beta
 *   is some perpendicular without meaning; the overall sign of either is unspecified); iterations [Q,n] int32 accepted
 *   steps; status [Q,n] int32: 0 converged, 1 iteration cap reached (the value is still no worse than the grid's: every
 *   accepted step improves), 2 not refined (flag bit 1: E and nu have poles; grid value and grid pair copied, 0
 *   iterations), -1 flag bit 0 or no grid winner (NaN).  The result is the stationary point of the basin the grid's
 *   winner lies in.  No atomics, no cross-lane traffic, nothing read back: bitwise reproducible, each row independent of the
 *   others, capturable.  tol > 0 finite, max_iter >= 0.
 * ------------------------------------------------------------------------------------------ */
int matten_elastic_props(const void* c, int is_fp64, int layout, int64_t n, double* voigt, double* compliance,
                         double* props, int32_t* flags, matten_stream_t stream);
int matten_elastic_props_bwd(const double* voigt, const double* compliance, const double* props, const int32_t* flags,
                             const double* g_props, const double* g_voigt, const double* g_compliance, int is_fp64,
                             int layout, int64_t n, void* g_c, matten_stream_t stream);
int matten_elastic_directional(const double* compliance, const int32_t* flags, const double* dirs, int64_t n,
                               int64_t n_dirs, double* young, double* beta, double* ext, int32_t* arg,
                               matten_stream_t stream);
int matten_elastic_pair(const double* compliance, const int32_t* flags, const double* dirs, const double* cos_sin,
                        int64_t n, int64_t n_dirs, int64_t n_angles, double* maps, double* ext, int32_t* arg,
                        matten_stream_t stream);
int matten_elastic_acoustic(const double* voigt, const int32_t* flags, const double* density, const double* dirs, int64_t n,
                            int64_t n_dirs, double modulus_unit, double* vel, double* ext, int32_t* arg, int32_t* n_unstable,
                            matten_stream_t stream);
int matten_elastic_directional_bwd(const double* compliance, const int32_t* flags, const double* dirs, int64_t n,
                                   int64_t n_dirs, const double* g_young, const double* g_beta, const double* g_ext,
                                   const int32_t* arg, double* g_compliance, matten_stream_t stream);
int matten_elastic_acoustic_bwd(const double* voigt, const int32_t* flags, const double* density, const double* dirs,
                                int64_t n, int64_t n_dirs, double modulus_unit, const double* g_vel, const double* g_ext,
                                const int32_t* arg, double* g_voigt, matten_stream_t stream);
int matten_elastic_refine(const double* compliance, const int32_t* flags, const double* dirs, const double* cos_sin,
                          const double* ext_dir, const int32_t* arg_dir, const double* ext_pair, const int32_t* arg_pair,
                          int64_t n, int64_t n_dirs, int64_t n_angles, double tol, int64_t max_iter, double* value,
                          double* vec_n, double* vec_m, int32_t* status, int32_t* iterations, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Kelvin moduli and mechanical stability (csrc/kelvin.hip, csrc/sym6.h): the eigen-decomposition of the 6x6 Mandel matrix
 * C^ = D C D, D = diag(1,1,1,sqrt2,sqrt2,sqrt2), of the symmetrised Voigt matrix C_IJ that matten_elastic_props writes
 * (pymatgen order xx, yy, zz, yz, xz, xy, no factors).  The Mandel map preserves the Frobenius norm of the rank-4 tensor,
 * so the eigenvalues of C^ are the six Kelvin moduli (eigen-stiffnesses; 3K once and 2G five times for an isotropic solid)
 * and its eigenvectors the eigenstrains.  fp64, one crystal per thread, cyclic Jacobi in registers, values in the units of
 * the input.
 * matten_elastic_kelvin: replaces diagonalising each ElasticTensor(t) the reference hands back (predict.py:217-218) on the
 *   host, one crystal at a time.
 *   voigt [n,36], flags [n] as matten_elastic_props wrote them (the mean of the two triangles is used) ->
 *   moduli [n,6] ascending; vectors [n,36] = the orthonormal U row-major, eigenvectors of C^ in its columns in the same
 *   order (the sign of a column is unspecified but deterministic), may be NULL; dilatation [n,6] = (tr eps_k)^2 / 3 in
 *   [0,1] (1: a purely volumetric mode, 0: an isochoric one; tr eps_k = U_0k + U_1k + U_2k), may be NULL.  The moduli are
 *   the same bits whichever of the two are asked for.  A row with flag bit 0, or with an entry of C^ that is not finite,
 *   is NaN in every output.
 * matten_elastic_kelvin_bwd: replaces autograd through a host eigvalsh per crystal.  The adjoint of the moduli from the
 *   forward's vectors (Jacobi is not run again): g_C^ = U diag(g_moduli) U^T, g_voigt [n,36] = D g_C^ D, every element
 *   written, symmetric.  A row with flag bit 0, or whose vectors are not finite, gets exact zeros whatever arrives
 *   (selects, not products).  Vectors and dilatation carry no gradient.  Exactly degenerate moduli: per-modulus gradients
 *   take the basis Jacobi left; a spectral function's gradient (sum_k h(l_k)) does not depend on it.
 * matten_elastic_kelvin_clamp: replaces the host loop eigh -> clip -> rebuild per crystal.  The tensor nearest to C in the
 *   Frobenius norm of the rank-4 tensor among those whose Kelvin moduli are all >= floor:
 *   out [n,36] = D^-1 U diag(max(l_k, floor)) U^T D^-1 from (moduli, vectors) as the forward wrote them, summed in the
 *   fixed order k = 0..5.  A row whose moduli are all >= floor is its 36 entries of `voigt` copied bit for bit (a select):
 *   `voigt` must be the symmetrised matrix matten_elastic_props wrote, or such a row comes back as unsymmetric as it came;
 *   a row with a NaN modulus is NaN.
 * All three: no atomics, no cross-lane traffic, nothing read back: bitwise reproducible, each row independent of the others,
 * capturable.  n = 0 is a no-op.  MATTEN_EINVAL: n < 0 or above 2^31 - 1 workgroups, a NULL required pointer with n > 0,
 * floor negative or not finite.
 * ------------------------------------------------------------------------------------------ */
int matten_elastic_kelvin(const double* voigt, const int32_t* flags, int64_t n, double* moduli, double* vectors,
                          double* dilatation, matten_stream_t stream);
int matten_elastic_kelvin_bwd(const double* vectors, const int32_t* flags, const double* g_moduli, int64_t n,
                              double* g_voigt, matten_stream_t stream);
int matten_elastic_kelvin_clamp(const double* voigt, const double* moduli, const double* vectors, double floor, int64_t n,
                                double* out, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Polycrystal bounds and the self-consistent estimate (csrc/polycrystal.hip): the bulk and shear modulus of an untextured
 * aggregate of equiaxed grains, beyond Voigt, Reuss and Hill -- the Hashin-Shtrikman (HS) bounds and the self-consistent
 * (SC; Kroener, Hershey, Willis) estimate, for any crystal symmetry.  Replaces a host loop over the ElasticTensor(t) objects
 * the reference hands back (predict.py:217-218).  Mandel form as above; u = (1,1,1,0,0,0)/sqrt3, J = u u^T, K_d = 1 - J,
 * iso(K,G) = 3K J + 2G K_d; c_J(T) = u^T T u, c_K(T) = (tr T - c_J(T)) / 5.  With the isotropic comparison medium (K0,G0),
 * Hill's polarisation tensor of a sphere in it, P = J / (3K0 + 4G0) + K_d 3 (K0 + 2G0) / (5 G0 (3K0 + 4G0)),
 * R = C^ - iso(K0,G0) and A = (1 + P R)^-1:
 *     F_K(C^; K0,G0) = c_J(C^ A) / 3 c_J(A)        F_G(C^; K0,G0) = c_K(C^ A) / 2 c_K(A)
 * (C0 -> 0: Reuss, C0 -> infinity: Voigt).  fp64, one crystal per thread, values in the units of the input.
 * matten_elastic_polycrystal:
 *   voigt [n,36], flags [n] as matten_elastic_props wrote them; moduli [n,6] (l_k, ascending), vectors [n,36] as
 *   matten_elastic_kelvin wrote them for that voigt (Jacobi does not run a second time; F is evaluated from the
 *   decomposition, no matrix is inverted).  out [n,6] = k_hs_lower, g_hs_lower, k_sc, g_sc, k_hs_upper, g_hs_upper;
 *   media [n,8] = the (K0, G0) of k_hs_lower, g_hs_lower, k_hs_upper, g_hs_upper, may be NULL (out is the same bits);
 *   status [n,2] int32 = status, iterations.
 *   SC: the fixed point (K,G) = F(C^; K,G) by plain iteration from the Voigt pair, until |dK| + |dG| <= sc_tol (K + G) or
 *   sc_max_iter applications of F; iterations counts the applications.
 *   HS: F is a lower bound on both moduli for every medium with C^ - iso(K0,G0) positive semi-definite, an upper bound
 *   for every medium with iso(K0,G0) - C^ so, and monotone in the medium, so the best media lie on the frontier of the
 *   feasible set, with w_k = (U_k . u)^2:
 *     lower: G0 in (0, l_min/2],        3K0 - 2G0 =  1 / sum_k w_k / (l_k - 2G0)
 *     upper: G0 in [l_max/2, infinity), 3K0 - 2G0 = -1 / sum_k w_k / (2G0 - l_k)
 *   Each of the four bounds is a one-dimensional search: a grid of hs_grid points (lower: G0 = (l_min/2)(1 - 1e-12) i/M,
 *   i = 1..M; upper: G0 = (l_max/2)(1 + 1e-12) 4^(i/(M-1)), i = 0..M-1), 60 golden-section steps in the bracket of the grid
 *   winner's two neighbours, the best point visited.  Every point visited is feasible: the result is a valid bound
 *   whatever the search does, the search decides only how tight it is.  The frontiers stop at l_min/2 and l_max/2 on
 *   purpose: beyond them feasible media exist only where the softest (stiffest) Kelvin mode carries dilatation.
 *   Row states: flag bit 0 or a decomposition that is not finite: every output NaN, status -1; flag bit 1 or l_min not > 0:
 *   every output NaN, status 2 (neither is defined); SC stopped at sc_max_iter: the last iterate, status 1; else status 0.
 * matten_elastic_polycrystal_bwd: replaces autograd through a host fixed-point loop.  The adjoint of (k_sc, g_sc) by the
 *   implicit-function theorem: g_C^ = (dF/dC^)^T l with (1 - dF/dx)^T l = g_sc [n,2], a 2x2 solve; dF/dC^ and dF/dx are
 *   analytic, from one Cholesky inverse of the positive definite C^ + P^-1 - iso(K,G) at the fixed point.  voigt, flags as
 *   the forward got them, out and status as it wrote them; g_voigt [n,36] = D g_C^ D, every element written, symmetric.
 *   A row with status -1 or 2 (or flag bit 0, or a value that is not finite) gets exact zeros by a select; a status-1 row
 *   is differentiated as if its last iterate were the fixed point.  The HS bounds carry no gradient: their medium sits
 *   on a constraint that moves with C^.
 * Both: no atomics, no cross-lane traffic, nothing read back: bitwise reproducible, each row independent of the others,
 * capturable.  n = 0 is a no-op.  MATTEN_EINVAL: n < 0 or above 2^31 - 1 workgroups, a NULL required pointer with n > 0,
 * hs_grid < 2, sc_tol not positive and finite, sc_max_iter < 1.
 * ------------------------------------------------------------------------------------------ */
int matten_elastic_polycrystal(const double* voigt, const int32_t* flags, const double* moduli, const double* vectors,
                               int64_t n, int hs_grid, double sc_tol, int sc_max_iter, double* out, double* media,
                               int32_t* status, matten_stream_t stream);
int matten_elastic_polycrystal_bwd(const double* voigt, const int32_t* flags, const double* out, const int32_t* status,
                                   const double* g_sc, int64_t n, double* g_voigt, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Textured polycrystals (csrc/texture.hip): the effective anisotropic tensor of an aggregate under an orientation
 * distribution -- the Voigt, Reuss, Hill and geometric (Matthies & Humbert) means.  Replaces a host loop over crystals x
 * orientations on the ElasticTensor(t) objects the reference hands back (predict.py:217-218).  A rotation R maps
 * crystal-frame to sample-frame components, C'_ijkl = R_ia R_jb R_kc R_ld C_abcd; an improper R acts like -R.  Mandel form
 * as above; N(R) = D Q(R) D^-1 (Q: Bond's matrix) is the orthogonal 6x6 matrix with C'^ = N C^ N^T.  A texture is G
 * orientations with weights normalised to sum 1; its operator is <X> = sum_g w_g N_g X N_g^T on symmetric 6x6 matrices.
 * An aggregate is a list of members (crystal, texture, volume fraction), fractions normalised per aggregate.  With
 * S^ = (C^)^-1 and L^ = log C^:
 *     voigt = sum_m f_m <C^_m>_t      reuss = (sum_m f_m <S^_m>_t)^-1      hill = (voigt + reuss) / 2
 *     geometric = exp(sum_m f_m <L^_m>_t)                                  (geometric(C)^-1 == geometric(S))
 * each returned as a Voigt stiffness matrix D^-1 X^ D^-1 (the convention of matten_elastic_props' voigt).  fp64.
 * matten_texture_operator: the cost of a texture must not depend on the number of crystals, so G orientations are reduced
 *   once to op [T,441]: op[t] acts on the 21 upper-triangle entries of a Mandel matrix in row-major order (0,0), (0,1), ...
 *   (0,5), (1,1), ... (5,5), X'_p = sum_q op[p,q] X_q, op[(I,J),(K,L)] = sum_g w_g (N_IK N_JL + [K != L] N_IL N_JK).
 *   R [G,9] row-major, weights [G] or NULL (equal), tex_ptr [T+1] int64: texture t owns orientations tex_ptr[t] ..
 *   tex_ptr[t+1]; tex_flags [T] int32.  A texture gets flag bit 0 and a NaN operator when it is empty (or its range is not
 *   inside 0..G), its weight sum is not positive, a weight is negative or not finite, or an R has a non-finite entry or
 *   max|R R^T - 1| > orth_tol.  A texture is cut into slices of slice_len orientations, one workgroup each (one thread
 *   per operator entry, the slice's N_g built 64 at a time into LDS); a slice adds its orientations in order, the partial
 *   sums go to workspace [T * ceil(G / slice_len) * 448] doubles and are added in slice order, then divided by the weight
 *   sum: fixed order, no atomics, bitwise reproducible for a given slice_len.  (Beyond the sketch of the issue: orth_tol,
 *   slice_len and the workspace are arguments.)
 * matten_texture_average: voigt [n,36], flags [n] as matten_elastic_props wrote them, moduli [n,6], vectors [n,36] as
 *   matten_elastic_kelvin wrote them for that voigt (Jacobi does not run on the inputs again: S^ = U diag(1/l) U^T,
 *   L^ = U diag(log l) U^T; the Voigt mean takes C^ from voigt itself).  op, tex_flags as above; member_crystal [M] int32,
 *   member_texture [M] int32, member_fraction [M]; agg_ptr [A+1] int64: aggregate a owns members agg_ptr[a] .. agg_ptr[a+1],
 *   added in list order.  out [A,4,36] = voigt, reuss, hill, geometric; status [A] int32.  The inverse of the mean
 *   compliance and the exponential of the mean logarithm are one cyclic Jacobi (csrc/sym6.h) each.  status -1 (all four
 *   NaN): a member with flag bit 0 or a decomposition that is not finite, a flagged member texture, a member index out of
 *   range, a fraction negative or not finite, a fraction sum not positive, an empty aggregate (or a range outside 0..M);
 *   status 2 (voigt computed, the other three NaN): a member with flag bit 1 or l_min <= 0; else 0.
 * matten_texture_average_bwd: g_out [A,4,36] -> g_voigt [n,36] = D g_C^ D, every element written, symmetric.  voigt: op^T g;
 *   reuss: g_S = -C_R g C_R, op^T, g_C = -S g_S S; hill: half of each; geometric: Daleckii-Krein at exp and at log,
 *   U (Delta o (U^T g U)) U^T with divided differences that stay finite at equal eigenvalues (log1p / expm1, a series below
 *   a relative gap of 1e-6).  The eigenvectors of the mean logarithm are those of the geometric mean in `out`, found by
 *   one Jacobi per aggregate.  Parts that the forward wrote as NaN contribute exact zeros (selects, not products); the
 *   voigt part of a status-2 aggregate still flows.  A crystal may belong to several aggregates: each member writes a row
 *   of 21, and crystal c adds the rows of members crystal_member[crystal_ptr[c] .. crystal_ptr[c+1]] (int32 / int64, the
 *   caller's inverse of member_crystal, ascending) in that order.  workspace: A * 64 + M * 21 doubles.  Textures, weights
 *   and fractions receive no gradient.  (Beyond the sketch: the inverse list and the workspace are arguments; voigt and
 *   flags are not needed.)
 * All three: no atomics, nothing read back, capturable; each aggregate independent of the others.  T = 0, A = 0 and n = 0
 * (bwd) are no-ops.  MATTEN_EINVAL: a negative count, n, M or A above 2^31 - 1 workgroups, T or T * slices above 2^31 - 1,
 * slice_len < 1, orth_tol negative or not finite, a NULL required pointer for a non-zero count; MATTEN_ENOMEM: a workspace
 * that is NULL or too small.  All checks return before anything touches a device.
 * ------------------------------------------------------------------------------------------ */
int matten_texture_operator(const double* R, const double* weights, const int64_t* tex_ptr, int64_t G, int64_t T,
                            double orth_tol, int64_t slice_len, double* workspace, int64_t workspace_doubles, double* op,
                            int32_t* tex_flags, matten_stream_t stream);
int matten_texture_average(const double* voigt, const int32_t* flags, const double* moduli, const double* vectors, int64_t n,
                           const double* op, const int32_t* tex_flags, int64_t T, const int32_t* member_crystal,
                           const int32_t* member_texture, const double* member_fraction, int64_t M, const int64_t* agg_ptr,
                           int64_t A, double* out, int32_t* status, matten_stream_t stream);
int matten_texture_average_bwd(const double* moduli, const double* vectors, int64_t n, const double* op, int64_t T,
                               const int32_t* member_crystal, const int32_t* member_texture, const double* member_fraction,
                               int64_t M, const int64_t* agg_ptr, int64_t A, const double* out, const int32_t* status,
                               const double* g_out, const int64_t* crystal_ptr, const int32_t* crystal_member,
                               double* workspace, int64_t workspace_doubles, double* g_voigt, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Group velocities, polarisations and phonon focusing (csrc/waves.hip): what the eigenvectors of the Christoffel matrix
 * give beyond the phase velocities of matten_elastic_acoustic.  fp64.
 * matten_elastic_waves: the launch shape of matten_elastic_acoustic -- one workgroup per crystal over unit directions dirs
 *   [n_dirs,3], the lanes striding the directions, the crystal's 21 constants read once.  voigt [n,36] (the mean of its two
 *   triangles is C_ijkl), flags [n], density [n], modulus_unit as there; s = modulus_unit / density.  Per direction n:
 *   Gamma_ik = C_ijkl n_j n_l, its eigenpairs (lambda_k, u_k), lambda ascending, k = 0, 1, 2, by the cyclic Jacobi of
 *   matten_elastic_acoustic_bwd (the eigenvalues are those of matten_elastic_acoustic); v_k = sqrt(lambda_k s).
 *   Unstable direction (an eigenvalue that is not positive and finite): every output of the direction is NaN and it is
 *   counted in n_unstable [n].  Degenerate mode: gap_k = min_{m != k} |lambda_k - lambda_m| / lambda_2 < deg_tol; the phase
 *   velocity of the branch is still written, everything else of it is NaN (undefined: conical refraction), and it is
 *   counted in n_degenerate [n,3] (modes of unstable directions are not).
 *   Polarisation: the unit vector u_k with u.n >= 0; where |u.n| <= 1e-9, u.e1 >= 0; where that is <= 1e-9 too, u.e2 >= 0,
 *   (e1, e2) the frame of n of matten_elastic_pair (e1 x e2 = n).  Longitudinal character (u_k.n)^2.
 *   Group velocity g_k = (s / v_k) P, P_j = C_ijml u_i u_m n_l (m/s; g_k.n = v_k); power-flow angle
 *   psi_k = acos(min(1, v_k / |g_k|)).  Focusing Jacobian J_k = g^ . (d_e1 g^ x d_e2 g^), g^ = g_k / |g_k|: the signed
 *   Jacobian of n -> g^ between unit spheres (1 / |J| is the phonon-focusing enhancement factor, infinite on a caustic; J < 0
 *   on a folded sheet), with the analytic derivative along e of (e1, e2):
 *     dGamma_ik = C_ijkl (e_j n_l + n_j e_l),  du = sum_{m != k} u_m (u_m^T dGamma u_k) / (lambda_k - lambda_m),
 *     dlambda = u_k^T dGamma u_k,  dv = s dlambda / (2 v_k),
 *     dP_j = C_ijml (du_i u_m + u_i du_m) n_l + C_ijml u_i u_m e_l  (two different du terms),
 *     dg = s dP / v_k - g dv / v_k,  dg^ = (dg - g^ (g^.dg)) / |g|.
 *   pol, group [n,n_dirs,3,3] (branch, component), scal [n,n_dirs,3,5] = v_k, |g_k|, psi_k, character, J_k: each optional,
 *   NULL = not written.  ext [n,6] = the largest psi of branch 0, 1, 2, then the smallest |J| of branch 0, 1, 2 over the
 *   directions; arg [n,6] int32 = their direction indices (NaN ignored, equal values resolved to the lowest index, NaN and
 *   -1 if no finite value).  Rows with flag bit 0 or a density that is not positive and finite: NaN in every floating-point
 *   output, -1 in every integer output.  No atomics; lane-strided, xor butterfly, waves in index order: bitwise
 *   reproducible.  Nothing is read back or allocated: capturable.
 *   MATTEN_EINVAL before any launch: n < 0 or > 2^31 - 1 (one workgroup per crystal), n_dirs < 1 or > (2^31 - 1) / 3, deg_tol negative or not finite, a NULL required
 *   pointer with n > 0; n == 0 returns MATTEN_OK.
 * ------------------------------------------------------------------------------------------ */
int matten_elastic_waves(const double* voigt, const int32_t* flags, const double* density, const double* dirs, int64_t n,
                         int64_t n_dirs, double modulus_unit, double deg_tol, double* pol, double* group, double* scal,
                         double* ext, int32_t* arg, int32_t* n_degenerate, int32_t* n_unstable, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Derived quantities of per-atom rank-2 tensors (predict.py:117-148: the reference hands back one 3x3 array per atom;
 * NMR users read the isotropic value, span and skew or the Haeberlen anisotropy and asymmetry off it, with the
 * principal axes).  fp64 arithmetic, one atom per thread, values in the units of the input.
 * matten_rank2_props:
 *   t [n,9] (= [n,3,3] row-major), fp32 (is_fp64 = 0) or fp64 (1).  The input is symmetrised first, A = (T + T^T)/2
 *   (shielding tensors are not symmetric); the isotropic part t = tr(A)/3 comes off before the cyclic Jacobi in
 *   registers (csrc/sym3.h) and is added back to the values: the axes and the scalars below are those of the deviator,
 *   resolved to eps span / gap however large the isotropic part is.  Eigenvalues ascending.
 *   vals [n,3] = l1 <= l2 <= l3; axes [n,9] = the orthonormal U row-major, eigenvectors in its columns in the same order
 *   (the sign of a column is unspecified but deterministic); axes may be NULL (= not written);
 *   props [n,5] = iso = (l1 + l2 + l3)/3, span = l3 - l1, skew = 3 (l2 - iso)/span (of the tensor as given: for a
 *   shielding tensor the Herzfeld-Berger kappa is its negative), zeta = l_z - iso (Haeberlen reduced anisotropy: z the
 *   principal value furthest from iso, l3 when skew <= 0 -- ties included -- else l1; y = 2, x the other extreme),
 *   eta = (l_y - l_x)/zeta in [0, 1];
 *   flags [n] int32: bit 0 = one of the nine inputs is not finite, every output of the row is NaN; bit 1 = span == 0
 *   exactly (a multiple of the identity): skew = eta = 0 by definition.
 * matten_rank2_props_bwd: the adjoint, from what the forward wrote (vals, axes, props, flags; the input is not kept and
 *   Jacobi is not run again).  g_vals [n,3], g_props [n,5] (fp64): the upstream gradients, each may be NULL (= zero).  With
 *   w = g_vals + sum_q g_props[q] dq/dl, d iso = (1,1,1)/3, d span = (-1,0,1), d skew = ((skew-1), 2, (-skew-1))/span,
 *   d zeta = e_z - (1,1,1)/3, d eta = (e_y - e_x)/zeta - (eta/zeta) d zeta:  g_t [n,9] = U diag(w) U^T in fp32
 *   (is_fp64 = 0) or fp64 (1), every element written, symmetric (it passes through the symmetrisation's transpose).  A row
 *   with flag bit 0 gets zeros whatever arrives (NaN included: selects, not products); a row with bit 1 ignores the
 *   upstream gradients of skew and eta.  The principal axes carry no gradient.  Exactly degenerate eigenvalues: the
 *   per-value gradients take the basis Jacobi left (finite; basis-dependent, as for matten_elastic_acoustic_bwd);
 *   symmetric functions (iso) do not depend on it.
 * Both: no atomics, no cross-lane traffic, nothing read back: bitwise reproducible, each row independent of the others,
 * capturable.  n = 0 is a no-op.  MATTEN_EINVAL: n < 0, is_fp64 outside {0, 1}, a NULL required pointer with n > 0.
 * ------------------------------------------------------------------------------------------ */
int matten_rank2_props(const void* t, int is_fp64, int64_t n, double* vals, double* axes, double* props, int32_t* flags,
                       matten_stream_t stream);
int matten_rank2_props_bwd(const double* vals, const double* axes, const double* props, const int32_t* flags,
                           const double* g_vals, const double* g_props, int is_fp64, int64_t n, void* g_t,
                           matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Rotations and symmetry of irreps tensors (the reference's own equivariance check, tests/model/test_tfn_tensor.py:98-139,
 * converts the prediction with utils.py:110-133 to_cartesian and rotates it on the host with a rank-4 einsum; here rows
 * stay in the irreps basis on the device).  fp64 arithmetic.  One convention for the harmonics, the Cartesian bases
 * (o3.cartesian_tensor_basis) and parity: for an orthogonal M the block of irrep (l, p) is
 *   D_{l,p}(M) = p^[det M < 0] D^l(det(M) M),   Y_l(R v) = D^l(R) Y_l(v) with the harmonics of csrc/sh.h.
 * matten_wigner_d:
 *   R [G,9] (= [G,3,3] row-major) fp64 -> D [G,165]: the blocks D^0..D^lmax (lmax <= 4) of the PROPER part det(M) M,
 *   row-major, at the offsets 0, 1, 10, 35, 84 of a row; the row stride is 165 whatever lmax, blocks above lmax are not
 *   written.  D^l = Y_l(R P) Y_l(P)^-1 over 2l+1 fixed unit vectors (constants of csrc/rotate.hip; the harmonics are
 *   restated there in fp64 and normalise their argument).
 *   flags [G] int32: bit 0 = an entry is not finite; bit 1 = max|M^T M - I| > orth_tol; bit 2 = det M < 0 (improper).
 *   A row with bit 0 or bit 1 is NaN throughout (its blocks up to lmax).
 * matten_irreps_rotate:
 *   out[r] = D(M_g) x[r] (transpose = 0) or D(M_g)^T x[r] (1, the adjoint), g = index[r], or with index = NULL g = 0
 *   (G == 1) or g = r (G == n).  x, out [n,dim] fp32 (is_fp64 = 0) or fp64 (1), rounded once on the store; out may be x.
 *   layout [K,4] int32 HOST rows (offset, mul, l, parity): mul copies of irrep (l, parity) from column `offset`, copy u at
 *   offset + u (2l+1); K <= 16; the rows' column ranges must be disjoint (overlapping rows are MATTEN_EINVAL: two thread
 *   groups would write the same columns).  Columns that no layout row covers are not written.  A row whose g lies outside [0, G) is
 *   NaN; a flagged rotation hands on the NaN of its D row.  D must hold the blocks up to the layout's largest l.
 * matten_irreps_average:
 *   out[r] = sum_j w_j D(M_op_idx[j]) x[r] / sum_j w_j over j in [op_ptr[r], op_ptr[r+1]), in list order; op_ptr [n+1]
 *   int64, op_idx [nnz] int32 into the G rows of D (shared: all cubic crystals of a batch point at the same 48 rows),
 *   weights [nnz] fp64 or NULL (= 1).  transpose = 1 applies every D^T: the adjoint with respect to x.
 *   The extra argument G (the rows of D) bounds op_idx.  The library cannot see nnz, so with G > 0 op_idx must be a valid
 *   pointer even when every list is empty (nnz = 0: any device word will do, it is not read; ops.irreps_average passes
 *   one); the caller vouches for op_ptr (ascending from 0, op_ptr[n] <= nnz).
 *   deviation [n] fp64 or NULL: |x[r] - out[r]|_2 / |x[r]|_2 from out as stored, 0 where x[r] = 0.
 *   An empty list is the trivial group: out = x, deviation 0.  A flagged operation (bit 0 or 1), an op_idx outside [0, G),
 *   a weight that is not finite or sum_j w_j not greater than 0: the row and its deviation are NaN.
 * All: no atomics, no allocation, nothing read back, sums in list order: bitwise reproducible and capturable.  n = 0 (and
 * G = 0 for the first two) is a no-op.  MATTEN_EINVAL without a launch: a negative size, lmax outside 0..4, K > 16, a
 * layout row with l > 4, parity outside +-1 or a block past dim, is_fp64 or transpose outside {0, 1}, index = NULL with G
 * neither 1 nor n, a NULL required pointer with n > 0.
 * ------------------------------------------------------------------------------------------ */
int matten_wigner_d(const double* R, int64_t G, int lmax, double orth_tol, double* D, int32_t* flags, matten_stream_t stream);
int matten_irreps_rotate(const void* x, int is_fp64, int64_t n, int64_t dim, const int32_t* layout, int K, const double* D,
                         const int32_t* flags, const int32_t* index, int64_t G, int transpose, void* out,
                         matten_stream_t stream);
int matten_irreps_average(const void* x, int is_fp64, int64_t n, int64_t dim, const int32_t* layout, int K, const double* D,
                          const int32_t* flags, int64_t G, const int64_t* op_ptr, const int32_t* op_idx,
                          const double* weights, int transpose, void* out, double* deviation, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Finding a crystal's symmetry (csrc/spacegroup.hip; the reference has no search of its own: it takes space groups from
 * pymatgen on the host).  fp64.  Per crystal: L = the cell (rows = lattice vectors), G = L L^T, a_max = the longest lattice
 * vector, f = pos L^-1, symprec a length in the units of the positions.  INTEGRATION.md, "Finding a crystal's symmetry",
 * has the definitions in full; matten_amd.symmetry.find_symmetry_host restates them in numpy.
 * matten_lattice_group:
 *   N_out [B,48,9] int8: the integer matrices N with |(N G N^T)_ij - G_ij| <= 2 symprec a_max for every entry, the identity
 *   first, then ascending in the nine entries row-major; n_lat [B] their number; slots from n_lat on are zero.  The rows of
 *   N are searched among |n_j| <= m_j = floor((a_max + symprec) |a*_j|), a*_j = column j of L^-1.
 *   flags [B]: MATTEN_SYM_NOT_FINITE (a non-finite entry or |det L| <= 1e-12), MATTEN_SYM_RANGE (an m_j > 4: hand in a
 *   reduced cell), MATTEN_SYM_AMBIGUOUS (more than 48 matrices pass: symprec is too large); each gives the identity only.
 * matten_crystal_symmetry:
 *   pos [N_total,3], cell [B,9], Z [N_total] int64, ptr [B+1] int64, pbc [B,3] bytes or NULL (all periodic), (N_in, n_lat,
 *   lat_flags) of matten_lattice_group at the same symprec.  Pivot atom p = the lowest-indexed atom of the species with the
 *   fewest atoms (ties: the smallest Z).  For lattice operation N and pivot-species atom j (ascending) the translation
 *   t = f_j - f_p N is accepted when every atom i has an atom k of its species with |(d - round(d)) L| <= symprec,
 *   d = f_i N + t - f_k; the first accepted j represents N.  Fractional rows transform as f' = f N + t, positions as
 *   r' = M r + t L with M = the polar factor of (L^-1 N L)^T.
 *   rot [B,48,9] (M), rot_int [B,48,9] int8 (N), trans [B,48,3] (t, wrapped to [-1/2, 1/2]), n_rot [B]: the accepted
 *   operations in lattice order; absent slots are zero.  src [48,N_total] int32: src[g,k] = the atom (global index) whose
 *   image under operation g lands on atom k; -1 in absent slots.  n_trans [B], ttrans [B,max_trans,3], tsrc
 *   [max_trans,N_total]: the same for the pure translations (N = identity, every accepted j, j = p first), of which the
 *   first max_trans are kept; n_trans counts all.
 *   flags [B]: lat_flags, and MATTEN_SYM_NOT_FINITE (a non-finite coordinate, no atoms), MATTEN_SYM_TOO_LARGE (more than
 *   MATTEN_SYM_MAX_ATOMS atoms), MATTEN_SYM_AMBIGUOUS (an accepted operation images two atoms onto one, or one atom has two
 *   images within symprec), MATTEN_SYM_NOT_PERIODIC (an open axis): each gives n_rot = n_trans = 1 and identity maps.
 *   MATTEN_SYM_TRUNC: n_trans > max_trans, the point group is complete, the translation list is not.
 * matten_irreps_average_atoms:
 *   out[k] = (1 / n_ops[b]) sum_{g < n_ops[b]} D(R_{b,g}) x[src[g,k]], b = row_struct[k], in the order of g; x, out [n,dim]
 *   fp32 or fp64 (out must not be x), layout as for matten_irreps_rotate, (D, flags) the table of matten_wigner_d over the
 *   B * G_cap rotations [B,G_cap,9], or D = NULL for identity blocks (the average over pure translations); src [G_cap,n].
 *   A source that is -1, outside [0, n) or of another crystal, a flagged D row (bit 0 or 1), an n_ops[b] outside 1..G_cap
 *   or a row_struct[k] outside [0, B): the row is NaN.
 * All: no atomics, no allocation, nothing read back, one writer per output word: bitwise reproducible and capturable.
 * MATTEN_EINVAL without a launch: a NULL required pointer, a negative count, max_trans < 1, symprec not positive and finite,
 * K > 16, a bad layout row, G_cap < 1, out == x.
 * ------------------------------------------------------------------------------------------ */
#define MATTEN_SYM_MAX_OPS 48
#define MATTEN_SYM_MAX_ATOMS 1024
#define MATTEN_SYM_NOT_FINITE 1
#define MATTEN_SYM_RANGE 2
#define MATTEN_SYM_TOO_LARGE 4
#define MATTEN_SYM_AMBIGUOUS 8
#define MATTEN_SYM_TRUNC 16
#define MATTEN_SYM_NOT_PERIODIC 32
int matten_lattice_group(const double* cell, int64_t B, double symprec, int8_t* N_out, int32_t* n_lat, int32_t* flags,
                         matten_stream_t stream);
int matten_crystal_symmetry(const double* pos, const double* cell, const int64_t* Z, const int64_t* ptr, const uint8_t* pbc,
                            int64_t B, int64_t N_total, double symprec, int max_trans, const int8_t* N_in,
                            const int32_t* n_lat, const int32_t* lat_flags, double* rot, int8_t* rot_int, double* trans,
                            int32_t* n_rot, int32_t* src, int32_t* n_trans, double* ttrans, int32_t* tsrc, int32_t* flags,
                            matten_stream_t stream);
int matten_irreps_average_atoms(const void* x, int is_fp64, int64_t n, int64_t dim, const int32_t* layout, int K,
                                const double* D, const int32_t* flags, int64_t B, int64_t G_cap, const int32_t* n_ops,
                                const int32_t* row_struct, const int32_t* src, void* out, matten_stream_t stream);


/* ==========================================================================================
 * Adjoint (backward) operators for the training step (reference: autograd through
 * model/model.py:276-372 shared_step -> loss.backward()).  fp32.
 * ========================================================================================== */

/* adjoint of matten_tp_paths (w_edge in the reference column order):
 *   dw[e,q]              = norm * sum_ijk C_ijk x[src,x_base+i] Y[e,y_off+j] G[dst,out_base+k]
 *   dx[src, x_base + i] += norm * w[e,q] * sum_jk C_ijk Y[e,y_off+j] G[dst,out_base+k]     (dx zero-initialised)
 *   col_meta[n_cols,4] int32 {x_base, out_base, nnz_begin, nnz_count | y_off<<16}; nnz_ijk[nnz,4] uint8 {i,j,k,0}
 *   (i-major per coupling); nnz_c[nnz] = sqrt(2 l3+1) C_ijk
 *   in_ptr[n_in+1] / in_cols[n_cols] (both or neither): the weight columns grouped by the input channel (x_base) they
 *   read.  With them a thread owns (edge, input channel) and adds its paths' contributions to dx in registers: one
 *   atomic per (edge, channel, component) instead of one per path; without, one thread per (edge, column). */
int matten_tp_backward(const float* x, int64_t d_in, const void* w_edge, int64_t w_ld, const float* sh_sorted,
                       int64_t sh_stride, const int32_t* src_sorted, const int32_t* dst_sorted,
                       const int32_t* col_meta, int64_t n_cols, const uint8_t* nnz_ijk, const float* nnz_c,
                       const float* g_agg, int64_t d_mid, float avg_num_neighbors, const float* num_neigh,
                       int64_t n_edges, float* dx, void* dw, int64_t dw_ld, const int32_t* in_ptr,
                       const int32_t* in_cols, int64_t n_in, int edge_is_bf16 /* w_edge AND dw are bf16 */,
                       matten_stream_t stream);

/* Adam (torch.optim.Adam semantics, amsgrad off, L2 weight decay added to the gradient) over ONE flat fp32 buffer of n
 * elements; step[0] (device) = the number of this step, already incremented by the caller; buffers 16-byte aligned. */
int matten_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const float* step,
                     float lr, float beta1, float beta2, float eps, float weight_decay, matten_stream_t stream);

/* The same step with its controls on the device: global 2-norm clipping of grads, a guard that skips a step whose gradient
 * is not finite, coupled (Adam) or decoupled (AdamW) weight decay, an exponential moving average of the parameters and a
 * learning rate read from device memory.  Enqueues at most three kernels on `stream` (sum of squares -> control -> update)
 * and nothing else: no read-back, no memset node, no second stream, so the call captures into a hipGraph and a replay
 * uses whatever ctl[0] holds at that moment.  All device state is the caller's:
 *   ctl      fp32 [8]   [0] learning rate (input)  [1] norm of grads at the last step  [2] scale applied to them
 *                       (both outputs; [1] is NaN when neither clipping nor the guard asked for the norm); rest zero
 *   counters int32 [2]  [0] steps skipped so far  [1] 1 if the last step was skipped, else 0
 *   step     fp32 [1]   number of steps taken; THIS call advances it (by 0 for a skipped step) -- unlike matten_adam_step
 *   workspace           matten_adam_ctl_workspace_bytes(n) bytes, 8-byte aligned: one fp64 partial per workgroup of the
 *                       norm pass.  The number of workgroups depends on n alone and every sum runs in a fixed order in
 *                       fp64 without atomics: the norm has the same bits on every device and in every run.
 * max_norm > 0: scale = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_); 0: no clipping.  guard != 0: a
 * non-finite sum of squares skips the step -- params, exp_avg, exp_avg_sq, ema and step keep their bits, counters[0] += 1.
 * Without the guard a non-finite norm makes scale, and so the parameters, NaN (as under torch).  With g' = scale * g:
 * decoupled == 0: g' += weight_decay * p, then matten_adam_step's rule; != 0: p *= 1 - lr * weight_decay first
 * (torch.optim.AdamW).  ema != NULL: ema = ema_decay * ema + (1 - ema_decay) * p_new in the same pass.
 * MATTEN_EINVAL: n < 0, beta1 / beta2 / ema_decay outside [0, 1), eps < 0, max_norm < 0 (or any of them NaN); for n > 0 a
 * NULL pointer other than ema, a flat buffer (ema included) off a 16-byte boundary, workspace_bytes below the query.
 * n == 0: MATTEN_OK, no pointer is looked at. */
size_t matten_adam_ctl_workspace_bytes(int64_t n);
int matten_adam_step_ctl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema /* or NULL */,
                         int64_t n, float* step, float* ctl, int32_t* counters, void* workspace, size_t workspace_bytes,
                         float max_norm, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                         int decoupled, int guard, matten_stream_t stream);

/* the same adjoint with the literal-coefficient coupling code of the forward kernels (cg_gen.h): a thread owns (edge,
 * channel of one input block) and walks the block's paths; one atomic per (edge, channel, component) into dx.
 *   blocks[n_blocks,4] int32 {x_off, mul, l1, first path | n_paths << 16}; paths[n_paths,4] {l1*25+l2*5+l3, w_off, out_off, 0};
 *   sum_lanes = sum over the blocks of mul rounded up to a power of two (sizes the launch: the blocks' workgroup ranges
 *   are laid end to end); w_edge / dw fp32, or both bf16 when edge_is_bf16
 * dx: two modes.  dx_edges == NULL: dx [N, d_in] zero-initialised, contributions meet through fp32 atomics (order not
 * fixed).  dx_edges != NULL (scratch [E, d_in]; every input block's columns are written, columns of input irreps without
 * a path must be zero on entry): each edge's contribution is stored and dx[n] = the sum over the edges leaving n in the
 * order of out_perm[out_ptr[n] .. out_ptr[n+1]) -- sorted-edge indices grouped by source node (the CSR of src_sorted:
 * matten_csr_build on it) -- bitwise reproducible; dx [n_nodes, d_in] need not be initialised.  With n_edges == 0 the
 * scratch has no bytes and may be NULL: dx is then zeroed whenever out_ptr is given. */
int matten_tp_backward_lit(const float* x, int64_t d_in, const void* w_edge, int64_t w_ld, const float* sh_sorted,
                           int64_t sh_stride, const int32_t* src_sorted, const int32_t* dst_sorted, const int32_t* blocks,
                           int64_t n_blocks, int64_t max_mul, const int32_t* paths, int64_t n_paths, const float* g_agg,
                           int64_t d_mid, float avg_num_neighbors, const float* num_neigh, int64_t n_edges, float* dx,
                           void* dw, int64_t dw_ld, int edge_is_bf16, int64_t n_nodes, const int32_t* out_ptr,
                           const int32_t* out_perm, float* dx_edges, int max_l, matten_stream_t stream);
/* matten_tp_backward_lit for training on the fused forward: w[E, W] is never read -- every workgroup re-evaluates the weights of
 * its (edges, input block) on the matrix cores from h2s[E, 2, 32] (matten_radial_hidden: the rows the forward used) and the
 * A fragments of the last radial layer in REFERENCE column order: frag / w_inv = matten_split_a_tiles over one pseudo-entry per
 * path (int32 [n_paths, 32], words 5 / 6 / 7 = w_off, first tile, ceil(mul / 16); plan.bw_w_entries), paths[p][3] = that first
 * tile.  Same dw / dx contract as matten_tp_backward_lit (fixed-order sums with out_ptr / out_perm / dx_edges). */
int matten_tp_backward_lit_wfree(const float* x, int64_t d_in, const uint16_t* h2s, const uint16_t* frag, const float* w_inv,
                                 const float* sh_sorted, int64_t sh_stride, const int32_t* src_sorted,
                                 const int32_t* dst_sorted, const int32_t* blocks, int64_t n_blocks, int64_t sum_lanes,
                                 const int32_t* paths, int64_t n_paths, const float* g_agg, int64_t d_mid,
                                 float avg_num_neighbors, const float* num_neigh, int64_t n_edges, float* dx, void* dw,
                                 int64_t dw_ld, int edge_is_bf16, int64_t n_nodes, const int32_t* out_ptr,
                                 const int32_t* out_perm, float* dx_edges, int64_t lds_floats, int max_l, int max_mul,
                                 matten_stream_t stream);
/* max_mul (w-free only): the channel count of the widest block; a workgroup holds 256 / (lanes per edge) edges, so blocks of more
 * than 256 channels are refused (MATTEN_EINVAL) -- such a layer runs matten_tp_backward_lit on a materialised w. */
/* max_l (both functions): the largest degree among the paths' (l1, l2, l3); <= 2 selects the instantiation without the l = 3, 4
 * coupling code (about half the registers, twice the resident waves). */
/* lds_floats (2048 .. 15360): floats of LDS per workgroup for its [edge][path][column] weight tile; a block whose paths do not
 * fit takes them in rounds (plan.bw_wfree_lds_floats = what the widest block needs in one round, capped at 4096). */
/* The third adjoint of the 'uvu' product (nn/utils.py:230-237,263, differentiated by autograd in the reference), w.r.t. the
 * edge harmonics:
 *   dy[e, l2^2 + j] = norm(dst_e) * sum_paths p sum_u w[e, w_off_p + u]
 *                       * sum_{i,k} C^{l1 l2 l3}_{ijk} x[src_e, x_off + u*D1 + i] * g_agg[dst_e, out_off_p + u*D3 + k]
 * with the same blocks / paths tables, the same scaled literals and the same max_l instantiations as
 * matten_tp_backward_lit.  A launch row owns the whole edge (lanes = channels, max_mul = the widest block's channel count
 * sizes them; wider blocks loop), one fixed-order cross-lane sum per edge, no atomics: bitwise reproducible.
 * dy [E, sh_stride] fp32, every column of every row written (zeros from (max_l <= 2 ? 9 : 25) on, and in the columns of
 * degrees no path reads); sh_stride >= that count.  w_edge fp32, or bf16 when edge_is_bf16. */
int matten_tp_backward_sh(const float* x, int64_t d_in, const void* w_edge, int64_t w_ld, const int32_t* src_sorted,
                          const int32_t* dst_sorted, const int32_t* blocks, int64_t n_blocks, int64_t max_mul,
                          const int32_t* paths, int64_t n_paths, const float* g_agg, int64_t d_mid, float avg_num_neighbors,
                          const float* num_neigh, int64_t n_edges, int edge_is_bf16, float* dy, int64_t sh_stride, int max_l,
                          matten_stream_t stream);

/* adjoint of matten_species_linear w.r.t. the packed weights (the adjoint w.r.t. x is matten_species_linear
 * itself with the transposed segment table and transposed packed weights):
 *   dWp[s, w_off + u*mo + w] = sum_{rows n of species s} sum_k x[n, x_off+u*d+k] dy[n, o_off+w*d+k]
 * fp32 MFMA over (row, component); fixed summation order.  Every weight of the table's segments is written (dwp need
 * not be initialised).  scratch [matten_species_linear_wgrad_scratch_floats(n_rows, n_species, w_stride)], required when
 * that count is above 0 (large batches: a species' rows are cut into slices of 128 rows; a species of several slices
 * writes one scratch row per slice and a second launch adds them in slice order), else may be NULL */
int matten_species_linear_wgrad(const float* x, int64_t d_in, const float* dy, int64_t d_out, const int32_t* order,
                                const int32_t* seg, int64_t n_species, int64_t n_rows, const int32_t* segs,
                                int64_t n_segs, int64_t w_stride, float* dwp, float* scratch, matten_stream_t stream);

/* adjoint of the Gate part of matten_gate_bn (bn_weight == NULL forward); every column of dx is written (no atomics:
 * a gate's gradient is summed over its channel's components in order) */
int matten_gate_bwd(const float* x, int64_t d_in, const int32_t* meta, int64_t d_out, const float* act_cst,
                    const float* dy, int64_t n_rows, float* dx, matten_stream_t stream);

/* e3nn BatchNorm in training mode (batch statistics over all rows; reference nn/utils.py:418,432-433):
 *   chan[n_chan,4] int32 {column offset, 2l+1, is_0e, index into bias / running_mean or -1}; col2chan[dim]
 *   fwd: mean[c] (0e only, else 0), nu[c] = mean_n mean_k (x-mean)^2, y = (x-mean) rsqrt(nu+eps) weight[c] (+ bias)
 *   bwd: dx (A, B are [n_chan] scratch that return sum dy (x-mean) and sum dy: dweight = A rsqrt(nu+eps), dbias = B) */
int64_t matten_bn_scratch_floats(int64_t n_rows, int64_t dim);
int matten_bn_train_fwd(const float* x, int64_t dim, int64_t n_rows, const int32_t* col2chan, const int32_t* chan,
                        int64_t n_chan, const float* weight, const float* bias, float eps, float* mean, float* nu,
                        float* y, float* running_mean, float* running_var, float momentum, float* scratch,
                        matten_stream_t stream);
/* scratch [matten_bn_scratch_floats(n_rows, dim)] (fwd and bwd; may be NULL when that is 0): large batches reduce in two
 * stages, per-(16-row block, column) partial records first, merged per channel in a fixed order (0e channels by the
 * pairwise mean / squared-deviation update, so no E[x^2] - mean^2 cancellation) */
/* running_mean [number of 0e channels] / running_var [n_chan] (both or neither, may be NULL): updated in place by the
 * statistics kernel, running = (1 - momentum) running + momentum batch (e3nn BatchNorm in training mode) */
int matten_bn_train_bwd(const float* x, const float* dy, int64_t dim, int64_t n_rows, const int32_t* col2chan,
                        const int32_t* chan, int64_t n_chan, const float* mean, const float* nu, const float* weight,
                        float eps, float* A, float* B, float* dx, float* dweight, float* dbias, float* scratch,
                        matten_stream_t stream);
/* dweight [n_chan] = A rsqrt(nu + eps), dbias [number of 0e channels] = B of the 0e channels (both or neither, may be NULL) */
/* Padded batches: the statistics, the running-average update and the adjoint's two reductions over the rows
 * [0, *n_valid) only, divided by *n_valid.  n_valid is a DEVICE word the kernels read (the host never does, so the call
 * captures and a replay sees the refreshed count); n_rows, the padded count, sizes the launches, the scratch and the
 * choice between the one-launch and the two-stage reductions.  Rows >= *n_valid get y from the valid rows' statistics
 * and dx = 0 exactly; nothing else depends on their contents.  *n_valid == n_rows gives the bits of the entries above.
 * *n_valid is clamped to [0, n_rows]; with no valid row mean and nu are zero and the running averages stay as they are.
 * MATTEN_EINVAL: as above, and a NULL n_valid. */
int matten_bn_train_fwd_valid(const float* x, int64_t dim, int64_t n_rows, const int32_t* col2chan, const int32_t* chan,
                              int64_t n_chan, const float* weight, const float* bias, float eps, float* mean, float* nu,
                              float* y, float* running_mean, float* running_var, float momentum, float* scratch,
                              const int64_t* n_valid, matten_stream_t stream);
int matten_bn_train_bwd_valid(const float* x, const float* dy, int64_t dim, int64_t n_rows, const int32_t* col2chan,
                              const int32_t* chan, int64_t n_chan, const float* mean, const float* nu, const float* weight,
                              float eps, float* A, float* B, float* dx, float* dweight, float* dbias, float* scratch,
                              const int64_t* n_valid, matten_stream_t stream);

/* e3nn NormActivation as the reference configures it (nn/utils.py:142-150: nonlinearity_type "norm"; normalize = True,
 * epsilon = 1e-8, bias = False): every channel c (chan[c] = {column offset, 2l+1, is_0e, mean index}, as for
 * matten_bn_train_fwd; every column of the row belongs to one channel) is scaled by f(n) / n with
 * n = sqrt(max(sum_k x_k^2, epsilon^2)) and f the activation code `act` (1 silu, 2 tanh, 3 sigmoid, 4 shifted softplus,
 * 5 abs) applied as is (no second-moment normalisation).  With bn_weight != NULL the eval-mode BatchNorm that follows
 * the activation is folded in (weight / sqrt(running_var + bn_eps) per channel, bias - running_mean * scale on 0e).
 * matten_norm_act_bwd: the adjoint without BatchNorm (a clamped norm is a constant). */
int matten_norm_act(const float* x, int64_t dim, int64_t n_rows, const int32_t* chan, int64_t n_chan, int act,
                    float epsilon, const float* running_mean, const float* running_var, const float* bn_weight,
                    const float* bn_bias, float bn_eps, float* y, matten_stream_t stream);
int matten_norm_act_bwd(const float* x, const float* dy, int64_t dim, int64_t n_rows, const int32_t* chan, int64_t n_chan,
                        int act, float epsilon, float* dx, matten_stream_t stream);

/* Backpropagation through the activation followed by eval-mode BatchNorm (frozen running statistics; the reference
 * gets it from autograd through e3nn's Gate / NormActivation, nn/utils.py:96-150, and its BatchNorm outside training,
 * nn/utils.py:414-418).  The forward is matten_gate_bn / matten_norm_act with the running statistics; nothing but x is
 * kept, the activated value a is re-evaluated.  One pass over x and dy writes every column of dx and, when dweight is
 * given, one partial record per (16-row block, column or channel); a second launch adds a channel's records in a fixed
 * order (no atomics, bitwise reproducible):
 *   dweight [n_chan] = sum dy (a - running_mean) / sqrt(running_var + eps),  dbias [number of 0e channels] = sum dy.
 * dweight == NULL: dx only (frozen affine), dbias / scratch / bn_chan are not touched.  running_mean / running_var /
 * bn_weight are only read.  scratch: the floats the _scratch_floats entry returns for (n_rows, d_out) (Gate) or
 * (n_rows, n_chan) (norm activation).  meta / act_cst as for matten_gate_bn, chan as for matten_norm_act; bn_chan
 * [n_chan,4] is the BatchNorm's channel table over the OUTPUT columns (as for matten_bn_train_fwd). */
int64_t matten_bn_eval_bwd_scratch_floats(int64_t n_rows, int64_t n_cols);
int matten_gate_bn_eval_bwd(const float* x, int64_t d_in, const int32_t* meta, int64_t d_out, const float* act_cst,
                            const int32_t* bn_chan, int64_t n_chan, const float* running_mean, const float* running_var,
                            const float* bn_weight, float eps, const float* dy, int64_t n_rows, float* dx, float* dweight,
                            float* dbias, float* scratch, matten_stream_t stream);
int matten_norm_act_bn_eval_bwd(const float* x, const float* dy, int64_t dim, int64_t n_rows, const int32_t* chan,
                                int64_t n_chan, int act, float epsilon, const float* running_mean,
                                const float* running_var, const float* bn_weight, float bn_eps, float* dx, float* dweight,
                                float* dbias, float* scratch, matten_stream_t stream);

/* Instance ("graph") normalisation, reference nn/utils.py:448-588 (the reference's own InstanceNorm: one set of
 * statistics per crystal, nodes as samples): matten_bn_train_fwd / _bwd with per-crystal statistics, in training and in
 * evaluation alike (it keeps no running averages).  Rows are grouped per crystal: seg_ptr[n_seg + 1] int64 row offsets,
 * seg_of_row[n_rows] int64 = the crystal of every row (the batch dict's `ptr` and `batch`).  chan as above, except that
 * the reference centres and biases every l = 0 channel (0e AND 0o: `ir.l == 0`, nn/utils.py:531,572), so chan[.][2]
 * is set for both.  mean / nu / A / B are [n_seg, n_chan]. */
int matten_instance_norm_fwd(const float* x, int64_t dim, int64_t n_rows, const int64_t* seg_ptr, const int64_t* seg_of_row,
                             int64_t n_seg, const int32_t* col2chan, const int32_t* chan, int64_t n_chan,
                             const float* weight, const float* bias, float eps, float* mean, float* nu, float* y,
                             matten_stream_t stream);
int matten_instance_norm_bwd(const float* x, const float* dy, int64_t dim, int64_t n_rows, const int64_t* seg_ptr,
                             const int64_t* seg_of_row, int64_t n_seg, const int32_t* col2chan, const int32_t* chan,
                             int64_t n_chan, const float* mean, const float* nu, const float* weight, float eps, float* A,
                             float* B, float* dx, matten_stream_t stream);

/* adjoint of matten_segment_reduce */
int matten_segment_reduce_bwd(const float* dy, int64_t dim, const int64_t* ptr, int64_t n_segments, int mean, float* dx,
                              matten_stream_t stream);


/* ==========================================================================================
 * Graph construction on the GPU (replaces neighbor_list_and_relative_vec,
 * data/data.py:285-413, i.e. ase.neighborlist.primitive_neighbor_list("ijS") + the self-edge filter).
 *   edges = all (i, j, S): | pos[j] + S.cell - pos[i] | < r_cut (strict, fp64), (i==j, S==0) excluded,
 *   emitted in lexicographic order (i, j, Sx, Sy, Sz); i, j are GLOBAL node ids (ptr-offset applied).
 *   pos[N,3] fp64; cell[B,9] fp64 (rows = lattice vectors); ptr[B+1] int64;
 *   pair_ptr[B+1] int64 = running sum of n_b^2: ordered atom pairs are numbered crystal by crystal, i-major.
 * matten_graph_prep (replaces the per-batch prologue of the reference's collate, data/dataset.py:150-152): per crystal
 *   the inverse cell in closed form, frac[N,3] = pos @ inv, bound[B,3] = r_cut |inv[:, k]| (a neighbour's shift
 *   along axis k lies within bound_k of -(frac_j - frac_i)_k), batch[N] int64, pos_f32[N,3], cell_f32[B,9].
 * Two passes: matten_neighbor_count -> counts[pair_ptr[B]] (edges of each ordered pair (i, j)); the caller scans
 * them into offsets[pair_ptr[B] + 1] (exclusive, int64); matten_neighbor_summary -> {n_edges, smallest edge count
 * of a crystal} (the builder's one read-back); matten_neighbor_fill writes edge_index[2,n_edges] (int64),
 * edge_cell_shift[n_edges,3] (fp32) and num_neigh[N] (fp32, optional: edges per centre atom, the reference's
 * bincount(i), data/data.py:401-411).  max_atoms = largest n_b; at most 65535 crystals per call.
 * The destination-sorted CSR of the list (what matten_csr_build derives from edge_index: destination = edge_index[1],
 * stable in the edge id) comes out of the same two passes when asked for: counts_t[pair_ptr[B]] (optional) receives each
 * pair's count at its j-major number pair_ptr[b] + (j - lo) n_b + (i - lo); the caller scans it into offsets_t like
 * offsets (offsets_t[0] is subtracted: the scan may continue the i-major one), and matten_neighbor_fill then also writes rowptr[n_atoms + 1], src_sorted[n_edges], perm[n_edges] (int32; all
 * four of offsets_t / rowptr / src_sorted / perm or none: NULL) -- bit for bit matten_csr_build's outputs.
 *
 * matten_graph_prep_pbc (reference data/data.py:285-413: neighbor_list_and_relative_vec(..., cell, pbc) hands a bool
 *   per axis to ASE): matten_graph_prep with pbc[B,3] (uint8, non-zero = periodic).  An open axis generates no image
 *   (S_k = 0); a cell row on an open axis may be zero and is not used by the search.  The cell is completed for the
 *   inverse (open rows := unit vectors orthogonal to the periodic rows); frac and bound are written as by
 *   matten_graph_prep on the periodic axes and as 0 on the open ones, which makes the search kernels walk exactly
 *   S_k = 0 there -- they take these outputs unchanged.  cell_f32 is the caller's cell.  singular[B] (int32) := 1 where
 *   the periodic vectors of a crystal are linearly dependent (|det| of the completed cell <= 1e-12; that crystal is
 *   searched as if open), and *n_singular (int64, zeroed by the caller) is incremented once per such crystal.
 * matten_neighbor_rows_count / matten_neighbor_rows_fill (reference data/data.py:285-413, same edge contract and the
 *   same canonical order): the search without per-pair bookkeeping, for large structures.  One wave per centre atom;
 *   batch[N] (int64, matten_graph_prep) names its crystal.  _count -> counts[n_atoms] (int32, edges of each centre
 *   atom); the caller scans them into offsets[n_atoms + 1] (exclusive, int64; matten_neighbor_summary with ptr in the
 *   place of pair_ptr gives the read-back); _fill writes edge_index[2,n_edges], edge_cell_shift[n_edges,3] and
 *   num_neigh[n_atoms] (optional).  No CSR is emitted here: matten_csr_build derives it.  n_atoms < 2^32.
 * matten_neighbor_cells_grid / _bin / _scatter / _count / _fill (reference data/data.py:285-413, same edge contract, the
 *   same canonical order and bit for bit the list of the rows entries): the rows search with a cell list in front, so
 *   that a centre atom tests the atoms of at most 27 bins instead of its whole crystal.  The bins only prune which j
 *   are looked at; whether an image is an edge is decided by the distance test all three routes share.
 *   _grid (one block per crystal; bound from matten_graph_prep; pbc[B,3] / singular[B] as for matten_graph_prep_pbc,
 *   NULL: every axis periodic / no singular cell) -> grid[B,8] int32 {bins along the three axes, 1 per open axis, 0, 0},
 *   grid_f64[B,16] {per axis: the column of the completed inverse, origin, bin width; used on open axes}, n_bins[B]
 *   int64.  Periodic axis k: nb = floor(1 / (bound_k (1 + 1e-6))) equal bins of frac - floor(frac), one bin when nb < 3.
 *   Open axis: bins at least r_cut |inv[:, k]| (1 + 1e-6) wide from the crystal's smallest pos . inv[:, k], no wrap.
 *   A crystal never gets more bins than it has atoms (the axis with the most bins is halved until that holds), so
 *   the sum of n_bins is at most n_atoms + n_crystals.  The caller scans n_bins into bin_base[B+1] (exclusive).
 *   _bin -> bin_of[n_atoms] (int32, bin within the crystal) and adds 1 per atom to bin_count[bin_base[B]] (int32,
 *   zeroed by the caller); the caller scans bin_count into bin_start[bin_base[B] + 1] (exclusive, int32); _scatter ->
 *   slot_atom[n_atoms] (int32: atom ids bin by bin, in no particular order inside a bin) and returns bin_count to zero.
 *   _count / _fill: as the rows entries.  _fill ranks the (j, count) records of a row, which a wave keeps in LDS;
 *   a row with more than matten_neighbor_cells_row_capacity() neighbouring atoms is walked as by the rows entry.
 *   matten_neighbor_cells_max_axis_bins(): the most bins _grid lays along one axis before the cap at the atom count (the
 *   host restatement data.graph.cell_grid_host clamps at the same number).  n_atoms < 2^31.
 * ========================================================================================== */
int matten_graph_prep(const double* pos, const double* cell, const int64_t* ptr, int64_t n_crystals, double r_cut,
                      double* frac, double* bound, int64_t* batch, float* pos_f32, float* cell_f32,
                      matten_stream_t stream);
int matten_graph_prep_pbc(const double* pos, const double* cell, const int64_t* ptr, const uint8_t* pbc,
                          int64_t n_crystals, double r_cut, double* frac, double* bound, int64_t* batch, float* pos_f32,
                          float* cell_f32, int32_t* singular, int64_t* n_singular, matten_stream_t stream);
int matten_neighbor_rows_count(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch,
                               const double* frac, const double* bound, double r_cut, int64_t n_atoms, int32_t* counts,
                               matten_stream_t stream);
int matten_neighbor_rows_fill(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch,
                              const double* frac, const double* bound, double r_cut, int64_t n_atoms,
                              const int64_t* offsets, int64_t n_edges, int64_t* edge_index, float* edge_cell_shift,
                              float* num_neigh, matten_stream_t stream);
int matten_neighbor_cells_row_capacity(void);
int matten_neighbor_cells_max_axis_bins(void);
int matten_neighbor_cells_grid(const double* pos, const double* cell, const int64_t* ptr, const double* bound,
                               const uint8_t* pbc, const int32_t* singular, int64_t n_crystals, double r_cut, int32_t* grid,
                               double* grid_f64, int64_t* n_bins, matten_stream_t stream);
int matten_neighbor_cells_bin(const double* pos, const double* frac, const int64_t* batch, const int32_t* grid,
                              const double* grid_f64, const int64_t* bin_base, int64_t n_atoms, int32_t* bin_of,
                              int32_t* bin_count, matten_stream_t stream);
int matten_neighbor_cells_scatter(const int64_t* batch, const int64_t* bin_base, const int32_t* bin_of,
                                  const int32_t* bin_start, int64_t n_atoms, int32_t* bin_count, int32_t* slot_atom,
                                  matten_stream_t stream);
int matten_neighbor_cells_count(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch,
                                const double* frac, const double* bound, const int32_t* grid, const int64_t* bin_base,
                                const int32_t* bin_of, const int32_t* bin_start, const int32_t* slot_atom, double r_cut,
                                int64_t n_atoms, int32_t* counts, matten_stream_t stream);
int matten_neighbor_cells_fill(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch,
                               const double* frac, const double* bound, const int32_t* grid, const int64_t* bin_base,
                               const int32_t* bin_of, const int32_t* bin_start, const int32_t* slot_atom, double r_cut,
                               int64_t n_atoms, const int64_t* offsets, int64_t n_edges, int64_t* edge_index,
                               float* edge_cell_shift, float* num_neigh, matten_stream_t stream);
int matten_neighbor_count(const double* pos, const double* cell, const int64_t* ptr, const double* frac,
                          const double* bound, const int64_t* pair_ptr, double r_cut, int64_t n_crystals,
                          int64_t max_atoms, int32_t* counts, int32_t* counts_t, matten_stream_t stream);
int matten_neighbor_summary(const int64_t* offsets, const int64_t* pair_ptr, int64_t n_crystals, int64_t* out2,
                            matten_stream_t stream);
int matten_neighbor_fill(const double* pos, const double* cell, const int64_t* ptr, const double* frac,
                         const double* bound, const int64_t* pair_ptr, double r_cut, int64_t n_crystals,
                         int64_t max_atoms, const int64_t* offsets, int64_t n_edges, int64_t* edge_index,
                         float* edge_cell_shift, float* num_neigh, const int64_t* offsets_t, int64_t n_atoms,
                         int32_t* rowptr, int32_t* src_sorted, int32_t* perm, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Rebuilding the edge list of the SAME atoms at new positions / cells without a host read (reference data/data.py:285-413,
 * same edge contract and canonical order): the pair search into buffers of fixed capacity, so that "new geometry -> edge
 * list -> forward" replays as one hipGraph.
 * matten_neighbor_scan (reference data/data.py:285-413: the running sums behind its edge order): offsets[n + 1] (int64) :=
 *   exclusive scan of counts[n] (int32), one block, no workspace: the caller's scan of matten_neighbor_count's counts
 *   (both halves at once, n = 2 pair_ptr[B], as the eager builder scans them) as a launch that captures.
 * matten_neighbor_fill_capped (reference data/data.py:285-413): matten_neighbor_fill's inputs without n_edges -- the
 *   kernels read E = offsets[pair_ptr[B]] from device memory -- plus the capacities (N_b, E_b, B_b) of the outputs;
 *   offsets_t is required.  It writes the padded batch layout of matten_batch_gather_padded (below): edge_index[2,E_b]
 *   (row stride E_b), edge_cell_shift[E_b,3], num_neigh[N_b], rowptr[N_b + 1], src_sorted[E_b], perm[E_b] and
 *   n_valid[3] = (n_atoms, E, n_crystals) (int64).  The E real edges and their destination-sorted CSR are
 *   matten_neighbor_fill's; behind them come the E_b - E padding edges in closed form: with K = B_b - n_crystals and
 *   P = N_b - n_atoms - (K - 1), padding node q < P owns the edges [floor(q (E_b - E) / P), floor((q + 1) (E_b - E) / P)),
 *   each q -> q with shift (1, 0, 0); num_neigh of a padding node is its degree, rowptr is closed over the padding nodes.
 *   The rows of pos, cell, atomic_numbers, batch and ptr are the caller's.
 *   flags[1] (int32, OR-ed in): MATTEN_CAPPED_OVERFLOW E > E_b; MATTEN_CAPPED_EDGELESS a real crystal without any edge;
 *   MATTEN_CAPPED_SINGULAR some singular[b] != 0 (matten_graph_prep_pbc's output; NULL: none).  With E > E_b NOTHING is
 *   stored but the flag: every output keeps the previous call's contents.  Every store is behind its capacity.
 *   MATTEN_EINVAL: what matten_neighbor_fill refuses, an empty batch, B_b <= n_crystals, N_b < n_atoms + (B_b -
 *   n_crystals), a capacity of 2^31 or more, a NULL output, flags or n_valid.
 * ------------------------------------------------------------------------------------------ */
#define MATTEN_CAPPED_OVERFLOW 1
#define MATTEN_CAPPED_EDGELESS 2
#define MATTEN_CAPPED_SINGULAR 4
int matten_neighbor_scan(const int32_t* counts, int64_t n, int64_t* offsets, matten_stream_t stream);
int matten_neighbor_fill_capped(const double* pos, const double* cell, const int64_t* ptr, const double* frac,
                                const double* bound, const int64_t* pair_ptr, double r_cut, int64_t n_crystals,
                                int64_t max_atoms, const int64_t* offsets, const int64_t* offsets_t, int64_t n_atoms,
                                const int32_t* singular, int64_t node_capacity, int64_t edge_capacity,
                                int64_t crystal_capacity, int64_t* edge_index, float* edge_cell_shift, float* num_neigh,
                                int32_t* rowptr, int32_t* src_sorted, int32_t* perm, int64_t* n_valid, int32_t* flags,
                                matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batch assembly from a device-resident training set (replaces PyG's collate at reference data/dataset.py:150-152,
 * which concatenates the picked crystals on the host for every batch of every epoch).
 *
 * A batch is a disjoint union with node and edge ranges in crystal order, so each of its arrays is the concatenation of
 * the picked crystals' rows, some with an offset added.  matten_batch_gather moves every array of a batch in ONE launch.
 *   table[5][n_crystals + 1] (int32, device), one column per picked crystal in batch order: destination node start,
 *     destination edge start, source node start, source edge start, source crystal.  The closing column holds
 *     (n_nodes, n_edges, 0, 0, 0).  The host derives it from its copies of the store's running sums.
 *   streams[n_streams][words] (int64, HOST memory, read before the call returns), words = MATTEN_BATCH_STREAM_WORDS
 *     here and MATTEN_BATCH_PAD_STREAM_WORDS for matten_batch_gather_padded, which reads the same six words first: per
 *     array {source pointer, destination pointer, element size (4 or 8), elements per row, class, operation}.
 *     class: whose rows these are (MATTEN_BATCH_NODE / _EDGE / _CRYSTAL).  Operation:
 *       RAW         the row copied as is, any class, any width (16-, 8- or 4-byte accesses as alignment allows)
 *       ADD32_NODE  int32 per edge + the crystal's destination node start      (source / destination ids in sorted order)
 *       ADD32_EDGE  int32 per edge + the crystal's destination edge start      (the two CSR permutations)
 *       ADD64_NODE  int64 per edge + the crystal's destination node start      (one row of edge_index)
 *       ROWPTR32    int32 per node + the destination edge start; the destination holds n_nodes + 1 entries, the last
 *                   one is set to n_edges                                      (the row pointers of the two CSRs)
 *       BATCH64     int64 per node: the crystal's position in the batch; no source
 *       PTR64       int64 per crystal: its destination node start; n_crystals + 1 entries, the last n_nodes; no source
 *   Sources hold the store's rows (crystal-relative ids); destinations hold n_nodes / n_edges / n_crystals rows.
 * MATTEN_EINVAL: a negative size, sizes of 2^31 or more, more than MATTEN_BATCH_MAX_STREAMS streams, a NULL table,
 * streams array, destination or (where the operation reads one) source, an element size other than 4 or 8, a row of no
 * elements, an unknown class or operation, an operation outside its class or element size, a pointer off its element size.
 * Up to matten_batch_gather_lds_rows() - 1 crystals the two destination running sums are searched in LDS, above that
 * in global memory.  No workspace, no atomics, no synchronisation.
 * ------------------------------------------------------------------------------------------ */
#define MATTEN_BATCH_MAX_STREAMS 32
#define MATTEN_BATCH_STREAM_WORDS 6
#define MATTEN_BATCH_NODE 0
#define MATTEN_BATCH_EDGE 1
#define MATTEN_BATCH_CRYSTAL 2
#define MATTEN_BATCH_OP_RAW 0
#define MATTEN_BATCH_OP_ADD32_NODE 1
#define MATTEN_BATCH_OP_ADD32_EDGE 2
#define MATTEN_BATCH_OP_ADD64_NODE 3
#define MATTEN_BATCH_OP_ROWPTR32 4
#define MATTEN_BATCH_OP_BATCH64 5
#define MATTEN_BATCH_OP_PTR64 6
int matten_batch_gather_lds_rows(void);
int matten_batch_gather_max_streams(void);
int matten_batch_gather(const int64_t* streams, int64_t n_streams, const int32_t* table, int64_t n_crystals,
                        int64_t n_nodes, int64_t n_edges, matten_stream_t stream);

/* The same batch grown to FIXED sizes, so that a captured training step can replay it: the same kernel, which behind
 * the v_crystals picked crystals (v_nodes nodes, v_edges edges, written as matten_batch_gather writes them: that entry is
 * this one without padding crystals) synthesises K = n_crystals - v_crystals >= 1 padding crystals from closed forms (no
 * source rows, no search, no second launch).
 *   Padding crystal 0 owns P = n_nodes - v_nodes - (K - 1) >= 1 nodes and all n_edges - v_edges padding edges; padding
 *   crystals 1 .. K-1 own one node and no edge.  Node j of padding crystal 0 owns the padding edges
 *   [floor(j Ep / P), floor((j + 1) Ep / P)), each a self-image edge j -> j, so the padding edges are destination-sorted:
 *   ADD32_EDGE streams get the identity there, ADD32_NODE / ADD64_NODE the owning node, ROWPTR32 the closed-form bounds,
 *   BATCH64 / PTR64 follow the layout.
 *   streams: words, classes and operations as above; words 7 and 8 are the fill of a RAW stream's padding rows and the
 *   fill's element (low four bytes for 4-byte elements):
 *       PAD_ZERO    zeros                         PAD_CONST   every element = value   (atomic_numbers)
 *       PAD_FIRST   (value, 0, 0, ...)            (edge_cell_shift = (1, 0, 0))
 *       PAD_DIAG3   value on the diagonal of a 3 x 3 row (cell = pad_length * I; 9 elements)
 *       PAD_DEGREE  one float per node: the number of padding edges it owns (num_neigh)
 *   table[5][n_crystals + 1]: the destination running sums cover the padding crystals; the closing column holds
 *   (n_nodes, n_edges, v_nodes, v_edges, v_crystals).  n_valid[3] (int64, device) receives its last three entries: the
 *   kernel copies them from the table, not from the arguments.
 * MATTEN_EINVAL: whatever matten_batch_gather refuses (one decoder reads the records of both), and
 * n_crystals <= v_crystals, n_edges < v_edges, n_nodes < v_nodes + (n_crystals - v_crystals), a negative valid size, a
 * NULL n_valid, an unknown fill, a fill on a stream that is not RAW, PAD_DEGREE off a one-float node stream, PAD_DIAG3
 * off a 9-element row.  Plain stores only: no atomics, no workspace. */
#define MATTEN_BATCH_PAD_STREAM_WORDS 8
#define MATTEN_BATCH_PAD_ZERO 0
#define MATTEN_BATCH_PAD_CONST 1
#define MATTEN_BATCH_PAD_FIRST 2
#define MATTEN_BATCH_PAD_DIAG3 3
#define MATTEN_BATCH_PAD_DEGREE 4
int matten_batch_gather_padded(const int64_t* streams, int64_t n_streams, const int32_t* table, int64_t n_crystals,
                               int64_t n_nodes, int64_t n_edges, int64_t v_crystals, int64_t v_nodes, int64_t v_edges,
                               int64_t* n_valid, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Loss over the selected atoms of a per-atom prediction (reference model/model.py:340-345: preds[atom_selector], then
 * the task's mean loss and mean-absolute-error metric, model/task.py:238-248).  Boolean indexing has a data-dependent
 * output shape (a host read per step, not capturable); here the selector is one int32 word per row, any nonzero value
 * = selected, and pred / target share the shape [n_rows, d] (fp32, contiguous; rows without a target hold anything).
 *   kind 0: squared error, kind 1: absolute error.
 *   sum   (fp64, device)  the per-element loss summed over the selected rows
 *   count (int64, device) the number of selected rows
 *   loss  (fp32, device)  sum / (count * d), rounded once; count == 0 gives 0 (a definition: the reference's mean over
 *                         nothing is NaN; a real batch has a selected atom, an all-padding row set stays finite)
 * Differences and squares are formed in fp64; the reduction runs in a fixed order (lane, wave butterfly, workgroup
 * through LDS, per-workgroup partials in index order): no floating-point atomics, two calls give the same bits.  A row
 * with selector 0 never enters the arithmetic (NaN / Inf there changes no output bit); a NaN in a selected row reaches
 * loss.  At most two launches (one up to matten_selected_loss_tile_elems() elements), no host read, no allocation.
 *   workspace: matten_selected_loss_workspace_bytes(n_rows, d) bytes, 8-byte aligned (0 bytes: may be NULL).
 * matten_selected_loss_bwd: grad_pred[i, c] = g * dl(pred - target) / (count * d) on selected rows (dl = 2x, or sign(x)
 * with sign(0) = 0), formed in fp64 and rounded once, and +0.0 on every other row; count == 0 writes zeros.  g (fp32)
 * and count (the forward's word) are read from device memory.  One elementwise launch.
 * MATTEN_EINVAL: n_rows < 0, d < 1, n_rows * d >= 2^31, kind outside {0, 1}, a NULL or misaligned pointer;
 * MATTEN_ENOMEM: a workspace smaller than the query.  Both before any launch.  n_rows == 0 writes (0, 0, 0).
 * ------------------------------------------------------------------------------------------ */
int matten_selected_loss_tile_elems(void);   /* elements (n_rows * d) one workgroup takes per round */
int matten_selected_loss_max_blocks(void);   /* workgroups of the forward at most; more elements are strided over */
size_t matten_selected_loss_workspace_bytes(int64_t n_rows, int64_t d);
int matten_selected_loss(const float* pred, const float* target, const int32_t* selector, int64_t n_rows, int64_t d,
                         int kind, double* sum, int64_t* count, float* loss, void* workspace, size_t workspace_bytes,
                         matten_stream_t stream);
int matten_selected_loss_bwd(const float* pred, const float* target, const int32_t* selector, int64_t n_rows, int64_t d,
                             int kind, const float* g, const int64_t* count, float* grad_pred, matten_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Loss and metric sums over the VALID rows of a padded crystal batch: the crystal-level twin of matten_selected_loss.
 * The real rows of pred / target ([n_rows, d], fp32, contiguous) are [0, *n_valid); n_valid is a device word (the B word
 * of a padded batch's `_amd_n_valid`, which the gather kernel writes and every replay of a captured step refreshes) and
 * is clamped to [0, n_rows].  One pass produces what a step's loss and its mean-absolute-error metric need:
 *   sums  (fp64 [2], device) sums[0] = sum (p - t)^2, sums[1] = sum |p - t| over the valid rows and their d columns
 *   count (int64, device)    the number of valid rows = clamp(*n_valid, 0, n_rows)
 *   loss  (fp32, device)     sums[kind] / (count * d), rounded once; count == 0 gives 0
 * Arithmetic, element order and reduction are matten_selected_loss's (the same kernels, another row predicate): with
 * selector[row] = (row < *n_valid) that entry gives the same bits for sums[kind], count and loss.  A row at or beyond
 * *n_valid is loaded but never enters the arithmetic (a select: NaN / Inf there changes no output bit).  At most two
 * launches, no floating-point atomics, no host read, no allocation.
 *   workspace: matten_valid_loss_workspace_bytes(n_rows, d) bytes, 8-byte aligned (0 bytes: may be NULL).
 * matten_valid_loss_bwd: grad_pred[i, c] = g * dl(pred - target) / (count * d) on valid rows (dl = 2x, or sign(x) with
 * sign(0) = 0), formed in fp64 and rounded once, and +0.0 on every other row; count == 0 writes zeros.  g (fp32) and
 * count (the forward's word) are read from device memory.  One elementwise launch.
 * MATTEN_EINVAL / MATTEN_ENOMEM: as matten_selected_loss, and a NULL or misaligned n_valid.  n_rows == 0 writes zeros.
 * ------------------------------------------------------------------------------------------ */
size_t matten_valid_loss_workspace_bytes(int64_t n_rows, int64_t d);
int matten_valid_loss(const float* pred, const float* target, const int64_t* n_valid, int64_t n_rows, int64_t d,
                      int kind, double* sums, int64_t* count, float* loss, void* workspace, size_t workspace_bytes,
                      matten_stream_t stream);
int matten_valid_loss_bwd(const float* pred, const float* target, const int64_t* n_valid, int64_t n_rows, int64_t d,
                          int kind, const float* g, const int64_t* count, float* grad_pred, matten_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MATTEN_HIP_H */
