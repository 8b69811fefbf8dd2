/*
 * deftet_hip.h — C ABI of libdeftet_hip.so, the MI355X (gfx950) implementation of
 * DefTet's per-tetrahedron hot path.
 *
 * Conventions (mirroring the reference's bindings):
 *   - plain pointers + sizes, no torch types; `stream` is a hipStream_t passed as void*
 *     (NULL = the legacy default stream);
 *   - device-pointer entry points: the CALLER allocates every input, output and
 *     workspace buffer ("caller allocates, callee fills", as check_condition_tet.cpp:31-48
 *     and the utils/lib run(...) functions do); nothing is allocated behind the caller's back;
 *   - every entry point returns 0 on success or a negative DEFTET_E* code; the message
 *     is available from deftet_last_error() (thread-local).  The reference's AT_ASSERTM
 *     shape/device checks (check_condition_tet.cpp:19-25) become DEFTET_EINVAL;
 *   - kernels are enqueued on `stream` and NOT synchronised (the reference launches on
 *     the default stream and does not synchronise either); the `_host` builder variants
 *     are synchronous because they return data in host memory, exactly like run.so;
 *   - THE WORKSPACE CONTRACT: an entry point with a `workspace` takes a device buffer that is not NULL, 256-byte
 *     aligned and at least its *_workspace_bytes(...) long, and refuses any other with DEFTET_EINVAL; the
 *     message names the entry point, the bytes needed and the bytes given.  The exceptions are stated where
 *     they apply: NULL selects the brute-force path of deftet_tri_dist_fwd*, deftet_nn_index* and
 *     deftet_face_edge_adj*; deftet_rowdot*, deftet_sqrt_rowsum_f32 and deftet_radix_sort ask for no alignment,
 *     deftet_scan for 16 bytes; a path of an entry that uses no workspace does not look at it.
 *
 * Paths in comments are relative to the reference checkout.
 */
#ifndef DEFTET_HIP_H_
#define DEFTET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEFTET_OK 0
#define DEFTET_EINVAL (-1)   /* bad argument (null pointer, negative size, misaligned, workspace too small) */
#define DEFTET_ELAUNCH (-2)  /* HIP runtime / kernel launch failure */
#define DEFTET_ENODEV (-3)   /* no usable gfx950 device */
#define DEFTET_ELIMIT (-4)   /* size exceeds what the float-encoded index outputs can represent (2^24) */

/* point-in-tet algorithm selector */
#define DEFTET_PIT_AUTO 0    /* uniform-grid binned, tet-centric, certified fused plane filter: DEFTET_PIT_WAVE for sparse query sets
                              * (n_query <= 0.6 n_tet), DEFTET_PIT_SLAB otherwise (deftet_point_in_tet_resolve_algo) */
#define DEFTET_PIT_BRUTE 1   /* scalar-tiled brute force: the algorithmic equivalent of the reference kernel */
#define DEFTET_PIT_EXACT 2   /* binned, box test + exact predicate on every candidate (no filter; independent cross-check) */
#define DEFTET_PIT_SLAB 3    /* per-lane walk of the global cell table, three candidates per wave-iteration (k_tet_scan_slab) */
#define DEFTET_PIT_WAVE 4    /* a wave stages the candidates of its 64 tets in LDS, filter-only per-tet setup (k_tet_scan_wave) */
#define DEFTET_PIT_PAIR 5    /* the same with two tets per lane: a wave stages once for 128 tets (k_tet_scan_pair; measured slower, never AUTO) */

/* 420: connected components of a triangle list, their measures and the mesh clean-up — deftet_mesh_components_i64,
 *      deftet_mesh_cleanup_count_i64, deftet_mesh_cleanup_fill_i64 with deftet_mesh_components_workspace_bytes,
 *      deftet_mesh_gather_fwd_f32 / _bwd_f32 (mesh_components.hip). */
/* 410: Loop subdivision of triangle surfaces — deftet_loop_topology_count_i64, deftet_loop_topology_fill_i64 with
 *      deftet_loop_topology_workspace_bytes, deftet_loop_subdivide_fwd_f32 / _bwd_f32 (loop_subdivide.hip). */
/* 400: iso-solid measures on the tets — deftet_tet_iso_fraction_fwd_f32 / _bwd_f32, deftet_tet_iso_measures_fwd_f32 / _bwd_f32 with
 *      deftet_tet_iso_measures_workspace_bytes (tet_iso_measure.hip). */
/* 390: field gradients on the tets — deftet_tet_field_gradient_fwd_f32 / _bwd_f32, deftet_tet_field_energies_fwd_f32 / _bwd_f32 with
 *      deftet_tet_field_energies_workspace_bytes, deftet_tet_to_vertex_fwd_f32 / _bwd_f32 (tet_field_grad.hip). */
/* 380: conforming selective tet refinement (red-green closure on edge marks) — deftet_tet_refine_mark_i64, deftet_tet_refine_count_i64,
 *      deftet_tet_refine_fill_f32 and deftet_tet_refine_workspace_bytes (tet_refine.hip).
 * 370: generalised winding numbers for inside tests on open meshes — deftet_winding_number_f32, its workspace size,
 *      deftet_winding_number_levels, deftet_winding_number_resolve_algo (winding_number.hip).
 * 360: pixel-aligned image-feature sampling for the single-image branch — deftet_image_sample_fwd_f32, deftet_image_cells_f32,
 *      deftet_image_sample_bwd_map_f32 / _bwd_uv_f32 / _bwd_global_f32 and their workspace size (image_sample.hip).
 * 350: connected components of the inside tets and the occupancy clean-up on them — deftet_tet_components_u8,
 *      deftet_occupancy_cleanup_u8 and their workspace size (tet_components.hip).
 * 340: a per-vertex field at located query points — deftet_tet_field_sample_fwd_f32 / _bwd_w_f32 / _bwd_field_f32 and their
 *      workspace size (tet_field_sample.hip).
 * 330: tet-centroid feature sampling straight from the vertices — deftet_tet_centroid_sample_fwd_f32 / _bwd_pos_f32 /
 *      _bwd_vertices_f32 and their workspace size (tet_centroid_sample.hip).
 * 320: marching tetrahedra on a per-vertex field — deftet_edge_vertex_csr_i32, deftet_marching_tets_count_f32 / _fill_f32 / _bwd_f32
 *      and their workspace sizes (marching_tets.hip).
 * 310: ground-truth preparation — deftet_mesh_voxelize_f32, deftet_voxel_pack_u8 / _unpack_u8, deftet_extract_odms_u8,
 *      deftet_project_odms_i32, deftet_voxel_fill_b32, deftet_voxel_surface_count_b32 / _fill_b32, deftet_face_edges_i32 and their
 *      workspace sizes (dataprep.hip).
 * 300: the wide-channel vertex aggregation — deftet_vertex_aggregate_f32 (vertex_aggregate.hip).
 * 290: the point-voxel operators — deftet_avg_voxelize_fwd_f32 / _bwd_f32, deftet_voxel_sample_fwd_f32, deftet_voxel_cells_f32 /
 *      _from_inds_i32, deftet_voxel_sample_bwd_vol_f32 / _bwd_pos_f32 and their workspace size (pointvoxel.hip).
 * 280: rendering straight from the vertices — deftet_face_vertex_csr_i32 (+ workspace size), deftet_project_vertices_fwd_f32 /
 *      _bwd_f32, deftet_face_gather_fwd_f32 / _bwd_f32 (render_vertices.hip).
 * 270: surface extraction from a per-tet occupancy — deftet_tet_face_neighbours_i64, deftet_surface_extract_count_f32 / _fill_f32,
 *      deftet_surface_weld_f32 and their workspace sizes.
 * 260: the evaluation metrics — deftet_point_mesh_distance_f32 / _scan_f32, deftet_sample_points_f32, deftet_nn_distance_f32,
 *      deftet_surface_metrics_f32 and their workspace sizes.
 * 250: the vertex Laplacian regulariser — deftet_vertex_adjacency_csr_i32 (an adjacency and its transpose as CSRs) with its
 *      workspace size, deftet_vertex_laplacian_fwd_f32 / _bwd_f32 and the forward's workspace size.
 * 240: the fused rasterize-and-composite operator — deftet_sparse_render_composite_fwd_f32 / _bwd_f32 and their workspace sizes.
 * 230: the indexed point-in-tet query — deftet_point_in_tet_indexed_f32, _indexed_scan_f32, _indexed_bwd_to_vertices_f32 take
 *      vertices + a tet index list instead of the gathered [B,T,4,3] tensor (outputs bit-identical to the dense entry points).
 * 221: round 6, second half — 8-byte hit records, deftet_point_in_tet_bwd_to_vertices_f32, deftet_put_host_ints.
 * 220: round 6 — deftet_tet_order_coherence_f32 (what the traversal-order decision is made on); the rasterizer bins into at most
 *      90 x 90 tiles and gives sliver faces a certified box (no interface change).
 * 210: round 5 — the *_ex_* point-in-tet entry points (traversal order, query box with its miss counts),
 * deftet_tet_spatial_order_f32, DEFTET_PIT_PAIR; the backward takes per-tet lists above 2 queries per tet.
 * 200: round 4.  (deftet_tet_energies_workspace_bytes(B) is gone: the forward needs ..._bytes2(B, T).  Algorithm ids other
 * than the DEFTET_PIT_* values above — the STAGED / ROWS / ... ids 2-11 of the round-2 library — are rejected with
 * DEFTET_EINVAL, never silently mapped.) */
int deftet_version(void);
/* Measurement aid (bench.py): streams n_bytes (rounded down to 32 KB) with a plain float4 kernel — mode 0 copies src to dst,
 * mode 1 only reads src (dst then needs one float per 32 KB).  *done (optional) = bytes streamed per direction. */
int deftet_bandwidth_probe(const void *src, void *dst, size_t n_bytes, int mode, size_t *done, void *stream);
const char *deftet_last_error(void);
/* number of HIP devices visible; negative code on failure */
int deftet_device_count(void);
/* Measurement hook (no reference counterpart; used by bench.py for the roofline figure):
 * select ONE kernel by name (e.g. "k_tet_scan"; ""/NULL = off); every launch of it is then
 * bracketed by hipEvents recorded on the launch stream.  deftet_profile_read synchronises
 * them and returns the summed duration in ms and the number of launches, then resets. */
int deftet_profile_select(const char *kernel_name);
int deftet_profile_read(double *total_ms, long long *count);

/* ---------------------------------------------------------------------------------
 * A1  point-in-tet occupancy query
 * replaces: layers/DefTet/check_condition_tetrahedron_base/check_condition_tet.cpp:31-48
 *           (dr_forward_batch) -> check_condition_tet_for.cu:124-216
 * tet  f32 [B,T,4,3] contiguous, 16-byte aligned;  pts f32 [B,Q,3];
 * cond f32 [B,Q] (= [B,Q,1]) receives the LOWEST tet index whose four same-side tests
 *      agree (check_condition_tet_for.cu:172-178), else -1;  fully overwritten.
 * bary f32 [B,Q,4] or NULL: barycentric weights of the hit tet by the formula of
 *      utils/tet_utils.py:28-45 (zeros for misses).
 * pred f32 [B,T] + occ f32 [B,Q] (both or neither): fused DefTet.paste_occ gather
 *      occ[b,q] = pred[b, max(index,0)] (layers/DefTet/deftet.py:132-136); cond keeps its -1s.
 * hit_buf int32 [deftet_point_in_tet_hits_ints(B,T,Q)], 16-byte aligned, or NULL (every algo but DEFTET_PIT_BRUTE): opaque
 *      per-tet records of the accepted queries; handing it to deftet_point_in_tet_bwd_f32 makes
 *      the backward free of atomics, lists and memsets.
 * ------------------------------------------------------------------------------- */
size_t deftet_point_in_tet_workspace_bytes(int n_batch, int n_tet, int n_query, int algo);
size_t deftet_point_in_tet_hits_ints(int n_batch, int n_tet, int n_query);
int deftet_point_in_tet_f32(const float *tet, const float *pts, float *cond, float *bary,
                            const float *pred, float *occ, int32_t *hit_buf,
                            int n_batch, int n_tet, int n_query, int algo,
                            void *workspace, size_t workspace_bytes, void *stream);

/* The same operator in two calls.  The QUERY side (bounding box + counting sort of the queries
 * into grid cells) depends only on pts and on the sizes, so it can be enqueued ahead of time —
 * e.g. on a second stream while the previous step's backward is still running — and the TET side
 * (traversal + finalize) consumes it.  One prepare feeds exactly ONE scan (the scan uses up the
 * result sentinels and counters that prepare resets); both calls must see the same pts, sizes,
 * algo (a binned one) and workspace, and the scan must be ordered after the prepare (same stream
 * or an event).  deftet_point_in_tet_f32 == prepare followed by scan on one stream. */
int deftet_point_in_tet_prepare_f32(const float *pts, int n_batch, int n_tet, int n_query, int algo,
                                    void *workspace, size_t workspace_bytes, void *stream);
int deftet_point_in_tet_scan_f32(const float *tet, const float *pts, float *cond, float *bary,
                                 const float *pred, float *occ, int32_t *hit_buf,
                                 int n_batch, int n_tet, int n_query, int algo,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* Traversal order (no reference counterpart: the reference scans all tets for every query, in index order).
 * The filter kernels stage the candidates of 64 CONSECUTIVE tets, so their speed — never their result — depends on how
 * coherently the caller's tet list is numbered.  The topology of a DefTet grid is static (layers/DefTet/deftet.py:65-68), so
 * a caller computes ONCE, from any positions of one shape, a permutation that walks the tets column by column
 * (deftet_tet_spatial_order_f32: tet f32 [T,4,3] -> order int32 [T]; breaks int32 [2] on the device, may be NULL, receives
 * how often the column changes or z jumps inside a group of 64 consecutive tets of the caller's order ([0]) and of the
 * computed one ([1]) — when [0] is not much larger than [1] the list is coherent as it is and NULL should be passed on) and
 * hands it to the *_ex_* variants below.  Every output (cond, bary, occ, hit_buf) is identical with and without it:
 * "lowest tet index" (check_condition_tet_for.cu:176-178) is decided on the original indices. */
size_t deftet_tet_spatial_order_workspace_bytes(int n_tet);
int deftet_tet_spatial_order_f32(const float *tet, int n_tet, int32_t *order, int32_t *breaks,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* How coherent a numbering is for the traversal (round 6; what hip_ops.auto_tet_order decides on, no stopwatch):
 * out2[0] = steps inside groups of 64 consecutive tets of `order` (int32 [T] on the device, or NULL = the caller's own
 * numbering) where the next tet's centroid lies more than three mean box extents from the one before, out2[1] = steps looked
 * at.  out2 receives two plain 4-byte stores and may be host-mapped memory.  tet: f32 [T,4,3] of ONE shape. */
size_t deftet_tet_order_coherence_workspace_bytes(int n_tet);
int deftet_tet_order_coherence_f32(const float *tet, int n_tet, const int32_t *order, int32_t *out2,
                                   void *workspace, size_t workspace_bytes, void *stream);
/* Query box (no reference counterpart either).  The binned algorithms span their cell grid over the box of the call's regular
 * queries, which a first launch measures.  query_box_in (f32 [B,6] = lo xyz, hi xyz on the device, or NULL) replaces the
 * measurement: the grid spans that box, enlarged by 1/32 per side, and the launch is not made.  It is a HINT, never a promise:
 * a query outside it is answered exactly by the side path that serves NaN / Inf / huge queries — at brute-force cost per such
 * query, so hand in the sampler's box (dataloader.py:108 draws from 1.05 (U - 0.5)) or what an earlier call with the same
 * distribution measured: query_box_in is read by the call's kernels: like any input it must not be written while they run (hand boxes from call to
 * call on ONE stream, or order the streams with an event).  query_box_out (f32 [B,6] or NULL; must not alias query_box_in) receives the box of THIS call's regular
 * queries (lo > hi when there is none).  query_box_misses (int32 [B] or NULL; any memory the device can write — host-mapped
 * memory lets the caller poll it without synchronising) receives, when query_box_in is given, the number of regular queries
 * of each shape that fell outside it (NaN / Inf / huge queries are not counted): a caller that reuses boxes sees there that its
 * query distribution moved and measures again (what hip_ops.point_in_tet(query_box="track") does).  Every output is identical
 * with and without a box. */
int deftet_point_in_tet_ex_f32(const float *tet, const float *pts, float *cond, float *bary,
                               const float *pred, float *occ, int32_t *hit_buf,
                               int n_batch, int n_tet, int n_query, int algo, const int32_t *tet_order,
                               const float *query_box_in, float *query_box_out, int32_t *query_box_misses,
                               void *workspace, size_t workspace_bytes, void *stream);
int deftet_point_in_tet_prepare_ex_f32(const float *pts, int n_batch, int n_tet, int n_query, int algo,
                                       const float *query_box_in, float *query_box_out, int32_t *query_box_misses,
                                       void *workspace, size_t workspace_bytes, void *stream);
int deftet_point_in_tet_scan_ex_f32(const float *tet, const float *pts, float *cond, float *bary,
                                    const float *pred, float *occ, int32_t *hit_buf,
                                    int n_batch, int n_tet, int n_query, int algo, const int32_t *tet_order,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* A1b  backward of the weights (the reference's own backward,
 * check_condition_tetrahedron_base/utils.py:55-58, returns None).
 * grad_w f32 [B,Q,4] -> grad_tet f32 [B,T,4,3] = d(sum grad_w*w)/d tet; grad_pts f32 [B,Q,3]
 * or NULL receives d/d pts.  accumulate == 0: grad_tet is fully overwritten (no pre-zeroing
 * needed); != 0: the result is added to its current content, like the reference's backward
 * kernels add into wrapper-zeroed buffers (tet_analytic_distance_batch/utils.py:65).
 * grad_occ f32 [B,Q] + grad_pred f32 [B,T] (both or neither): fused backward of the paste_occ
 * gather, grad_pred[b,t] = sum of grad_occ over the queries that pasted from t (misses -> tet 0).
 * hit_buf (from the forward, same tet/pts/cond) selects the fastest path (with grad_pred it
 * also needs 80*n_batch floats of workspace): every tet adds the queries of its record in ascending query
 * order — no atomics, the same bits on every run; else workspace
 * (deftet_point_in_tet_bwd_workspace_bytes) enables the linked-list gather path (per-tet lists threaded with one
 * atomic exchange per hit, added in arrival order); with neither a float-atomic scatter is used.  The records are for
 * the sparse case (BASELINE: 0.4 to 1 query per tet): with more than 2 queries per tet (n_query > 2 n_tet) records
 * overflow by the hundred, the list path is the faster one (measured) and, given a workspace of that size, runs even
 * when hit_buf is handed in. */
/* Diagnostics (not on the hot path): 8 int32 per shape left in `workspace` by the last forward — [0] irregular tets,
 * [1] irregular queries, [2] hit-record overflow flag, [5] tets re-scanned exactly, [6] overflowed tets, others unused.
 * Copies to host memory and synchronises the stream.  deftet_point_in_tet_grid_dims reports the cell grid (y/z cells per
 * axis, x cells) the binned algos use for a problem size. */
int deftet_point_in_tet_grid_dims(int n_tet, int n_query, int *cells_yz, int *cells_x);
/* the algorithm `algo` runs for a problem size (resolves DEFTET_PIT_AUTO; any other id is returned unchanged) */
int deftet_point_in_tet_resolve_algo(int algo, int n_tet, int n_query);
int deftet_point_in_tet_read_stats(const void *workspace, size_t workspace_bytes, int n_batch, int n_tet, int n_query, int algo,
                                   int32_t *out_host_8xB, void *stream);

size_t deftet_point_in_tet_bwd_workspace_bytes(int n_batch, int n_tet, int n_query);
int deftet_point_in_tet_bwd_f32(const float *tet, const float *pts, const float *cond,
                                const float *grad_w, float *grad_tet, float *grad_pts,
                                const float *grad_occ, float *grad_pred, const int32_t *hit_buf,
                                int n_batch, int n_tet, int n_query, int accumulate,
                                void *workspace, size_t workspace_bytes, void *stream);

/* DefTet.paste_occ (layers/DefTet/deftet.py:132-136): out[b,q] = pred[b, max(cond[b,q],0)];
 * cond itself is clamped in place like the reference does (condition[condition<0]=0) when
 * clamp_cond_inplace != 0.  Backward: grad_pred[b,t] += sum_q grad_out[b,q]. */
int deftet_paste_occ_fwd_f32(const float *pred_bxt, float *cond_bxq, float *out_bxq,
                             int n_batch, int n_tet, int n_query, int clamp_cond_inplace, void *stream);
int deftet_paste_occ_bwd_f32(const float *cond_bxq, const float *grad_out_bxq, float *grad_pred_bxt,
                             int n_batch, int n_tet, int n_query, int zero_grad_pred, void *stream);

/* Per-shape loss scalars: out[r] = sum_c a[r,c]*b[r,c] (b == NULL: row sums).  Deterministic
 * reduction; the values every rank all-gathers in the multi-GPU harness. */
size_t deftet_rowdot_workspace_bytes(int n_rows);
int deftet_rowdot_f32(const float *a, const float *b, float *out, int n_rows, long long n_cols,
                      void *workspace, size_t workspace_bytes, void *stream);
/* Two terms of different width in one launch pair:
 * out[r] = sum_c a[r,c]*b[r,c] + sum_c a2[r,c]*b2[r,c]  (a2 == NULL: first term only). */
int deftet_rowdot2_f32(const float *a, const float *b, long long n_cols, const float *a2, const float *b2,
                       long long n_cols2, float *out, int n_rows, void *workspace, size_t workspace_bytes,
                       void *stream);
/* out[r] = sum_c sqrt(x[r,c] + eps), n_rows <= 1024, one launch (workspace: deftet_rowdot_workspace_bytes), and its
 * backward grad_x[r,c] = grad_out[r] / (2 sqrt(x[r,c] + eps)).  The reference's surface terms end in
 * "sqrt(d^2 + 1e-10)" followed by the mean over the points (utils/mesh_utils.py:14, layers/DefTet/deftet.py:168-181):
 * this is that tail for the point-to-surface term, per shape. */
int deftet_sqrt_rowsum_f32(const float *x, float eps, float *out, int n_rows, long long n_cols, void *workspace,
                           size_t workspace_bytes, void *stream);
int deftet_sqrt_rowsum_bwd_f32(const float *x, float eps, const float *grad_out, float *grad_x, int n_rows,
                               long long n_cols, void *stream);
/* n HOST integers (per-shape counts, offsets) written to device arrays (any of out_i32 / out_i64 / out_f32, each [n] or NULL)
 * by a kernel that carries them in its argument block: asynchronous — unlike a copy from pageable host memory, which blocks
 * the host until the stream has drained — and legal inside a graph capture. */
int deftet_put_host_ints(const long long *host_values, int n, int32_t *out_i32, long long *out_i64, float *out_f32, void *stream);

/* ---------------------------------------------------------------------------------
 * A2-A6  adjacency builders.  Device variants take device pointers and a caller
 * workspace; `_host` variants keep the EXACT signature of the reference's
 * `extern "C" void run(...)` (plus an int status) so utils/lib/<lib>/interface.py can be
 * pointed at this library unchanged.
 * ------------------------------------------------------------------------------- */
size_t deftet_builder_workspace_bytes(int n_point, int n_tet);

/* replaces utils/lib/tet_adj_share/run.cpp:40-97.  out int32 [8*n_tet,3] rows
 * [t0,t1,f0],[t1,t0,f1] in ascending face-key order; *n_out = shared faces (rows/2). */
int deftet_tet_adj_share_i32(const int32_t *tet_list, int32_t *out_rows, int32_t *n_out_dev,
                             int n_point, int n_tet, void *workspace, size_t workspace_bytes, void *stream);
int deftet_tet_adj_share_host(int *tet_list, int *face_edge_p, int *n_face_edge_p, int n_point, int n_tet);

/* replaces utils/lib/tet_face_adj/run.cpp:18-92.  rows [fa,fb]; capacity in rows
 * (the reference sizes it 4*n_tet*50, interface.py:27-28).  wrap32 != 0 reproduces the
 * native 32-bit edge key (run.cpp:39); 0 follows the Python twin utils/tet_utils.py:155-201. */
int deftet_tet_face_adj_i32(const int32_t *tet_list, int32_t *out_rows, long long capacity_rows,
                            long long *n_out_dev, int n_point, int n_tet, int wrap32,
                            void *workspace, size_t workspace_bytes, void *stream);
int deftet_tet_face_adj_host(int *tet_list, int *face_edge_p, int *n_face_edge_p, int n_point, int n_tet);

/* replaces utils/lib/tet_point_adj/run.cpp:20-56.  out int32 [12*n_tet,2], unique directed
 * vertex pairs sorted by (a,b) (the reference order is libstdc++ hash order — unspecified). */
int deftet_tet_point_adj_i32(const int32_t *tet_list, int32_t *out_edges, int32_t *n_out_dev,
                             int n_point, int n_tet, void *workspace, size_t workspace_bytes, void *stream);
int deftet_tet_point_adj_host(int *tet_list, int *edge_p, int *n_edge, int n_point, int n_tet);

/* replaces utils/lib/colaps_v/run.cpp:39-59 ("%.5f" decimal-string keys, first occurrence wins). */
int deftet_colaps_v_f32(const float *point_nx3, int32_t *map_array, int32_t *inverse_idx,
                        int32_t *n_colaps_dev, int n_point, void *workspace, size_t workspace_bytes, void *stream);
int deftet_colaps_v_host(float *point_p, int *map_array_p, int *inverse_idx_p, int *n_colaps_v_p, int n_point);

/* replaces the pure-Python utils/tet_utils.py:208-256 (with_boundary=0) and
 * diff_render/diftet_6_subdiv/3_model/prepare_for_wz.py:49-104 (with_boundary=1).
 * Outputs int64, capacity 4*n_tet rows each, first-seen order; counts[3] (device int32) =
 * {n_face, n_boundary, n_multi}. */
int deftet_tet_to_face_i32(const int32_t *tet_list, int64_t *face_fx3, int64_t *tetidx_fx2,
                           int64_t *tetfaceidx_fx2, int64_t *boundary_fx3, int32_t *counts_dev,
                           int n_point, int n_tet, int with_boundary,
                           void *workspace, size_t workspace_bytes, void *stream);

/* Per-tet neighbour table [T,4] (-1 padded; partners in the order of the shared faces' positions in the unique-face
 * table) = the second return value of diff_render/diftet_6_subdiv/3_model/utils_tetsv.py:16-75 (tet_adj_share), and,
 * optionally, the per-tet-face owner table [4T,2] of utils/tet_utils.py:259-300 (tet_to_face_withtet; NULL = skip).
 * Inputs are the tetidx/tetfaceidx tables of deftet_tet_to_face_i32(with_boundary=1) (n_face rows). */
size_t deftet_tet_neighbours_workspace_bytes(int n_tet);
int deftet_tet_neighbours_i64(const int64_t *tetidx_fx2, const int64_t *tetfaceidx_fx2, int n_face, int n_tet,
                              int64_t *nbr_tx4, int64_t *withtet_4tx2, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * A7  DefTet.get_boundary_index (mode 1) / get_internal_index (mode 2), layers/DefTet/deftet.py:186-203.
 * face_fx3, tetidx_fx2 int64 (tet_to_face outputs), occ f32 [B,T].  out_rows int64 [B*F,3] receives
 * the selected faces of all shapes back to back in row-major mask order (boundary faces flipped
 * when the first tet is the occupied one); offsets int32 [B+1] (device) = start row of every shape. */
size_t deftet_boundary_index_workspace_bytes(int n_batch, int n_face);
int deftet_boundary_index_i64(const int64_t *face_fx3, const int64_t *tetidx_fx2, const float *occ_bxt,
                              int64_t *out_rows, int32_t *offsets, int n_batch, int n_tet, int n_face, int mode,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * Surface extraction: the triangle surface of a per-tet occupancy.
 * Local face i of tet (A,B,C,D) has the corners (a,b,c) = ([A,B,C,D][i], [B,A,D,C][i], [C,D,A,B][i]); rows come in ascending
 * (tet, local face) order per shape, shapes back to back.
 *
 * deftet_tet_face_neighbours_i64: nbr[t][i] = the tet across LOCAL FACE i of t, -1 when no other tet owns the face — what row t
 * of the i-th sparse matrix of tet_adj_share holds (utils/lib/tet_adj_share/run.cpp:40-97,
 * diff_render/diftet_6_subdiv/3_model/utils_tetsv.py:16-75).  Inputs: the tetidx / tetfaceidx tables of
 * deftet_tet_to_face_i32(with_boundary=1).  Either output may be NULL; the int32 table is what the kernels below read
 * (16 bytes per tet, 16-byte aligned).  Needs no workspace. */
int deftet_tet_face_neighbours_i64(const int64_t *tetidx_fx2, const int64_t *tetfaceidx_fx2, int n_face, int n_tet,
                                   int64_t *nbr_tx4, int32_t *nbr32_tx4, void *stream);

#define DEFTET_SX_BINARY 0     /* utils/tet_utils.py:427-471: n >= 0 && occ[n] != occ[t] && occ[t] == 1 (fp32; grid-boundary faces never) */
#define DEFTET_SX_THRESHOLD 1  /* utils_tetsv.py:79-128: fabs((double)no - (double)occ[t]) > htres && occ[t] > (float)(2 htres), no = 0 at the boundary */

/* Count pass (replaces the masks of utils/tet_utils.py:434-444 and utils_tetsv.py:88-101, 158-171).  The occupancy is either
 * occ_bxt f32 [B,T], or — occ_bxt NULL — the maximum of the four corner weights of weights_bxv f32 [B,n_vertex] through
 * tet_idx_tx4 int32 [T,4] (3_model/deftet.py:522-523; NaN propagates as in np.max).  offsets int32 [B+1] (device): first row of
 * every shape, offsets[B] = rows of the batch; all -1 if a neighbour or vertex index is out of range.  The workspace keeps the
 * per-workgroup row bases (and the fused occupancy): hand the SAME, untouched workspace to the fill pass. */
size_t deftet_surface_extract_workspace_bytes(int n_batch, int n_tet, int with_vertex_weights);
int deftet_surface_extract_count_f32(const float *occ_bxt, const float *weights_bxv, const int32_t *tet_idx_tx4, int n_vertex,
                                     const int32_t *nbr32_tx4, int n_batch, int n_tet, int mode, double htres, int32_t *offsets,
                                     void *workspace, size_t workspace_bytes, void *stream);
/* Fill pass (replaces the boolean-mask gathers of utils/tet_utils.py:447-470 and utils_tetsv.py:103-126, 173-223), same mode,
 * htres, neighbours and occupancy as the count pass (occ_bxt NULL = the occupancy the count pass fused from the vertex weights).
 * The count pass records in the workspace which of the two occupancies it ran on; a fill pass asked for the OTHER one (or handed a
 * workspace no count pass wrote) writes no row.
 * capacity = rows the outputs hold (offsets[B]).  face f32 [F,3,3]; with attr_bxtx4xc f32 [B,T,4,n_attr] (1 <= n_attr <= 8) also
 * face_attr f32 [F,3,n_attr]; index int64 [F,2] = (tet, local face) or NULL; faces int64 [F,3] = the corners' vertex ids from
 * tet_idx_tx4 or NULL. */
int deftet_surface_extract_fill_f32(const float *tet_bxtx4x3, const float *attr_bxtx4xc, int n_attr, const float *occ_bxt,
                                    const int32_t *tet_idx_tx4, const int32_t *nbr32_tx4, int n_batch, int n_tet, int mode,
                                    double htres, long long capacity, float *face, float *face_attr, int64_t *index, int64_t *faces,
                                    void *workspace, size_t workspace_bytes, void *stream);
/* Welded mesh of one shape (no reference counterpart: utils/tet_utils.py:474 leaves it to trimesh): the vertices some face uses,
 * renumbered in ascending original id.  n_out int32 [2] (device) = {n_used, 1 if a face id is outside [0, n_vertex)};
 * old_id int64, verts_out f32 [.,3], attr_out f32 [.,n_attr] (with attr_vxc) hold capacity >= min(n_vertex, 3 n_face) rows;
 * faces_out int64 [n_face,3] = the new ids. */
size_t deftet_surface_weld_workspace_bytes(int n_vertex);
int deftet_surface_weld_f32(const int64_t *faces_fx3, long long n_face, const float *verts_vx3, const float *attr_vxc, int n_attr,
                            int n_vertex, int capacity, int32_t *n_out, int64_t *old_id, float *verts_out, float *attr_out,
                            int64_t *faces_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * Connected components of a per-tet occupancy (350; tet_components.hip).  The reference leaves this to trimesh on
 * the host ("use trimesh to fix the surface": utils/tet_utils.py:474, utils/mesh_utils.py:259,270, 3_model/utils_tetsv.py:132,229).
 * inside_bxt uint8 [B,T] (non-zero = inside); nbr32_tx4 int32 [T,4] as above (16-byte aligned), shared by the shapes and taken
 * as undirected: tets t and u of one shape are connected when both are inside and u stands in row t or t in row u.
 * Per shape: labels int32 [B,T] = -1 outside, otherwise the SMALLEST tet index of the component (independent of the schedule);
 * sizes int32 [B,T] = tets of the component at its label's index, 0 elsewhere; open uint8 [B,T] = 1 at the label's index when a
 * tet of the component has a -1 entry in its row (the component reaches the grid boundary), 0 elsewhere; count int32 [B] =
 * components of the shape.  bad int32 [1] (device) = neighbour entries outside [-1, n_tet): counted, never followed (it also
 * counts a parent chain or a retry loop that ran out of its trip bound: neither can happen).  n_batch <= 65535,
 * n_batch * n_tet < 2^31.  Integer atomics only: the same bits on every run. */
size_t deftet_tet_components_workspace_bytes(int n_batch, int n_tet);
int deftet_tet_components_u8(const uint8_t *inside_bxt, const int32_t *nbr32_tx4, int n_batch, int n_tet, int32_t *labels, int32_t *sizes,
                             uint8_t *open, int32_t *count, int32_t *bad, void *workspace, size_t workspace_bytes, void *stream);
/* The clean-up, one device sequence without a read-back, in this order: (1) fill_voids: the components of the COMPLEMENT are
 * labelled and every one whose open flag is 0 becomes inside; (2) the filled mask is labelled; (3) min_size = m > 0 drops the
 * components with fewer than m tets; (4) keep_largest keeps the component with the most tets among those left, the smaller label
 * among equal sizes (an empty shape stays empty).  keep uint8 [B,T] = 0 / 1.  labels, sizes, open and count are optional, all or
 * none: the components of step (2), the labelling the selection was made on.  Same workspace size as above. */
int deftet_occupancy_cleanup_u8(const uint8_t *inside_bxt, const int32_t *nbr32_tx4, int n_batch, int n_tet, int keep_largest,
                                int min_size, int fill_voids, uint8_t *keep, int32_t *labels, int32_t *sizes, uint8_t *open,
                                int32_t *count, int32_t *bad, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * Conforming selective refinement of a tet list (380; tet_refine.hip): refine the selected tets and close the
 * refinement so that no split tet leaves a midpoint on an edge or face its neighbour still owns whole.  The reference's selective
 * generate_subdivision (3_model/prepare_for_wz.py:255-301 with subdiv_sig) does leave them.  Over edges_ex2 int64 [n_edge,2] and
 * tet_edge_tx6 int64 [n_tet,6] of deftet_tet_edges_i64 (local slots 0 ab, 1 ac, 2 ad, 3 bc, 4 bd, 5 cd), n_edge <= 6 n_tet:
 *   marks    every edge of a selected tet; then, until nothing changes, a tet's face with two of its three edges marked gets the
 *            third (faces as slots {0,1,3}, {0,2,4}, {1,2,5}, {3,4,5}).  The least fixed point of a monotone rule: the same set
 *            in whatever order the rule is applied.  A closed tet has 0, 1, 2 (opposite: slots e and 5 - e), 3 (one face) or 6
 *            marked slots: these are the only sets of slots in which no face has exactly two (all 64 checked), whatever ids
 *            tet_edge holds.  Any other pattern means the marks are not closed and is reported in bad;
 *   vertices marked edge number r in list order becomes vertex n_point + r = (x[a] + x[b]) / 2.0f;
 *   tets     in parent order, the children of one parent contiguous; "v[i] = m" is the parent with corner i replaced by m, m(p,q)
 *            the midpoint of the edge between corners p and q:
 *              0 marks  the parent;
 *              1 mark   edge (p,q), p < q: v[q] = m; v[p] = m;
 *              2 marks  edges e0 < e1 with ends (p0,q0), (p1,q1): {v[q0] = m0, v[q1] = m1}; {v[q0] = m0, v[p1] = m1};
 *                       {v[p0] = m0, v[q1] = m1}; {v[p0] = m0, v[p1] = m1};
 *              3 marks  the face's corners p < q < r: {v[q] = m(p,q), v[r] = m(p,r)}; {v[p] = m(p,q), v[r] = m(q,r)};
 *                       {v[p] = m(p,r), v[q] = m(q,r)}; {v[p] = m(p,q), v[q] = m(q,r), v[r] = m(p,r)};
 *              6 marks  the eight children of deftet_subdivide_f32, in its order.
 * Selecting every tet gives deftet_subdivide_f32's points, features and tets bit for bit; selecting none, the input.
 *
 * deftet_tet_refine_mark_i64: marks_e uint32 [n_edge], the caller's, one 0 / 1 word per edge.  reset != 0: the marks and *bad are
 * zeroed and the edges of the tets with select_t uint8 [n_tet] != 0 are marked; reset == 0 continues on the marks as they are
 * (select_t is not read).  Then n_sweeps (0..64) in-place sweeps, one tet per lane: marks only go 0 -> 1, no lane waits for
 * another, integer atomics only.  sweep_counts int32 [n_sweeps] (device) = the marks each sweep set; a sweep that set nothing
 * read a state nobody wrote during it, so a last count of 0 proves closure — call again while it is not 0 (every such sweep sets
 * a mark, so n_edge + 1 sweeps always suffice).  *bad (device) = 1 for a tet_edge entry outside [0, n_edge): such a tet is skipped. */
int deftet_tet_refine_mark_i64(const int64_t *tet_edge_tx6, const uint8_t *select_t, int n_tet, int n_edge, int reset, int n_sweeps,
                               uint32_t *marks_e, int32_t *sweep_counts, int32_t *bad, void *stream);
/* Count pass on closed marks: totals int32 [3] (device) = {M marked edges, T' tets of the refinement, bad}; bad = 1 for an illegal
 * pattern, a tet_edge entry outside [0, n_edge) or a marked edge with an end outside [0, n_point) (such a tet is counted as one
 * child: the sizes stay valid, the result is not a refinement).  Leaves the ranks and child offsets in the workspace for the fill
 * pass: hand the same workspace, untouched, to it. */
size_t deftet_tet_refine_workspace_bytes(int n_tet, int n_edge);
int deftet_tet_refine_count_i64(const int64_t *tet_edge_tx6, const int64_t *edges_ex2, const uint32_t *marks_e, int n_point, int n_tet,
                                int n_edge, int32_t *totals, void *workspace, size_t workspace_bytes, void *stream);
/* Fill pass, n_split = M and n_tet_new = T' of the count pass: points_new f32 [n_point+M,3], feat_new f32 [n_point+M,n_feat]
 * (n_feat = 0: not touched), tet_new int64 [T',4], parent int64 [T'], kind uint8 [T'] = the parent's number of marked slots,
 * edges_split int64 [M,2] = the ends of the marked edges. */
int deftet_tet_refine_fill_f32(const int64_t *tet_tx4, const int64_t *tet_edge_tx6, const int64_t *edges_ex2, const uint32_t *marks_e,
                               const float *points, const float *feat, int n_point, int n_tet, int n_edge, int n_feat, int n_split,
                               long long n_tet_new, float *points_new, float *feat_new, int64_t *tet_new, int64_t *parent,
                               uint8_t *kind, int64_t *edges_split, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * Marching tetrahedra on a per-vertex field (320; marching_tets.hip): a welded iso-surface mesh per shape, with
 * the gradient of its vertices.  A corner is inside iff field > iso (fp32, strict; NaN is outside).  Every edge of the unique
 * edge list whose ends differ gets one vertex, t = (iso - f_min) / (f_max - f_min), p = p_min + t (p_max - p_min) with min / max
 * = the edge's lower / higher vertex id; attributes use the same t.  Faces: per tet the triangles of its case code
 * sum(inside_k << k) as crossing-edge ids mapped to vertex rows, starting at the lowest local edge id, normals from the inside
 * to the outside corners of a positively oriented tet (a negatively oriented tet comes out flipped; nothing is detected).
 * Rows per shape: vertices in ascending edge id, faces in ascending tet id.
 *
 * deftet_edge_vertex_csr_i32: the vertex -> edge-end CSR of edges_ex2 int64 [n_edge,2] (deftet_tet_edges_i64): offsets int32
 * [n_vertex+1], slots int32 [2 n_edge] holding 2*e+side (side 0 = min) in ascending order per vertex; *bad_flag = 1 for an index
 * outside [0, n_vertex). */
size_t deftet_edge_vertex_csr_workspace_bytes(int n_vertex, int n_edge);
int deftet_edge_vertex_csr_i32(const int64_t *edges_ex2, int32_t *offsets, int32_t *slots, int32_t *bad_flag, int n_vertex, int n_edge,
                               void *workspace, size_t workspace_bytes, void *stream);
/* Count pass.  field_bxv f32 [B,n_vertex]; edges_ex2 int32 [n_edge,2] (8-byte aligned), tet_idx_tx4 int32 [n_tet,4] (16-byte
 * aligned), both with every index inside [0, n_vertex) (the caller's topology object has checked them).  Writes edge_vertex_bxe
 * int32 [B,n_edge] = the vertex row of the edge inside its shape, -1 where it does not cross, and offsets_2xb1 int32 [2,B+1]
 * (device) = first vertex row / first face row of every shape, [.][B] = the totals.  The workspace keeps the scanned counts:
 * hand the SAME, untouched workspace to the fill pass.  n_batch * (n_edge + 2 n_tet) must stay below 2^31 - 1 (the int32 row sums of
 * the one scan both counts share) and n_batch * n_vertex below 2^31; both passes check it. */
size_t deftet_marching_tets_workspace_bytes(int n_batch, int n_tet, int n_edge);
int deftet_marching_tets_count_f32(const float *field_bxv, const int32_t *edges_ex2, const int32_t *tet_idx_tx4, int n_batch, int n_vertex,
                                   int n_tet, int n_edge, float iso, int32_t *edge_vertex_bxe, int32_t *offsets_2xb1, void *workspace,
                                   size_t workspace_bytes, void *stream);
/* Fill pass, same field, iso and lists.  n_vert / n_face = rows the outputs hold (the totals of the count pass).  verts f32
 * [n_vert,3]; with attr_bxvxc f32 [B,n_vertex,n_attr] (1 <= n_attr <= 8; NULL with n_attr = 0) vert_attr f32 [n_vert,n_attr];
 * faces int64 [n_face,3] = vertex rows local to the shape; optional edge_id int64 [n_vert], t f32 [n_vert], tet_id int64 [n_face]. */
int deftet_marching_tets_fill_f32(const float *pos_bxvx3, const float *field_bxv, const float *attr_bxvxc, int n_attr,
                                  const int32_t *edges_ex2, const int32_t *tet_idx_tx4, const int32_t *tet_edge_tx6,
                                  const int32_t *edge_vertex_bxe, int n_batch, int n_vertex, int n_tet, int n_edge, float iso,
                                  long long n_vert, long long n_face, float *verts, float *vert_attr, int64_t *faces, int64_t *edge_id,
                                  float *t, int64_t *tet_id, void *workspace, size_t workspace_bytes, void *stream);
/* Backward: grad_verts f32 [n_vert,3] and / or grad_vert_attr f32 [n_vert,n_attr] (either may be NULL = zero) to grad_pos f32
 * [B,n_vertex,3], grad_field f32 [B,n_vertex], grad_attr f32 [B,n_vertex,n_attr] (each may be NULL).  One thread per (b,v) walks
 * the vertex's CSR row in slot order and skips the edges whose edge_vertex entry is -1: (1-t) g or t g into grad_pos / grad_attr,
 * dt/df (g_p . (p_max - p_min) + g_a . (a_max - a_min)) into grad_field with dt/df_min = (iso - f_max) / (f_max - f_min)^2,
 * dt/df_max = -(iso - f_min) / (f_max - f_min)^2.  Sums in double in a fixed order, no atomics: the same bits on every run;
 * exact zeros for vertices without a crossing edge.  edge_vertex_bxe and offsets_2xb1 are what the count pass wrote.  n_batch <= 65535
 * (the batch is the grid's second dimension). */
int deftet_marching_tets_bwd_f32(const float *grad_verts, const float *grad_vert_attr, long long n_vert, const float *pos_bxvx3,
                                 const float *field_bxv, const float *attr_bxvxc, int n_attr, const int32_t *edges_ex2,
                                 const int32_t *csr_offsets, const int32_t *csr_slots, const int32_t *edge_vertex_bxe,
                                 const int32_t *offsets_2xb1, int n_batch, int n_vertex, int n_edge, float iso, float *grad_pos,
                                 float *grad_field, float *grad_attr, void *stream);

/* ---------------------------------------------------------------------------------
 * N1  ground-truth occupancy by ray parity:
 *   kal.ops.mesh.check_sign(verts, faces, points, hash_resolution=512)
 * (layers/DefTet/deftet.py:46, eval.py:239, dataloader.py:92).  PARITY UNPINNED — Kaolin is not in
 * the reference tree; the contract (ray along +x, Moller-Trumbore in fp32, eps 1e-7, odd number of
 * crossings = inside) is oracle/deftet_oracle_sign.c, which the kernels match bit for bit.
 * verts f32 [B,V,3]; faces int64 [F,3] (shared by the batch, like Kaolin); points f32 [B,N,3];
 * inside uint8 [B,N] (0/1); count int32 [B,N] or NULL (number of crossings); *bad_flag (device
 * int32) = 1 if a face index is outside [0,V).  algo: DEFTET_CS_AUTO = faces binned in the (y,z)
 * plane (exact, certified like the tets), DEFTET_CS_BRUTE = every point against every face.
 * --------------------------------------------------------------------------------- */
#define DEFTET_CS_AUTO 0
#define DEFTET_CS_BRUTE 1
size_t deftet_check_sign_workspace_bytes(int n_batch, int n_face, int algo);
int deftet_check_sign_f32(const float *verts, const int64_t *faces, const float *points, uint8_t *inside,
                          int32_t *count, int32_t *bad_flag, int n_batch, int n_vertex, int n_face, int n_point,
                          int algo, void *workspace, size_t workspace_bytes, void *stream);
/* The same for a DIFFERENT mesh per shape (layers/DefTet/deftet.py:44-47 loops over the batch):
 * verts_cat f32 [sum V_b,3] and faces_cat int64 [sum F_b,3] (vertex indices local to their shape) are
 * the meshes back to back, vert_offsets / face_offsets int32 [B+1] (device) their row offsets;
 * n_face_total = sum F_b, n_face_max = max F_b.  One launch sequence for the whole batch. */
size_t deftet_check_sign_ragged_workspace_bytes(int n_batch, long long n_face_total, int n_face_max, int algo);
int deftet_check_sign_ragged_f32(const float *verts_cat, const int32_t *vert_offsets, const int64_t *faces_cat,
                                 const int32_t *face_offsets, const float *points, uint8_t *inside,
                                 int32_t *count, int32_t *bad_flag, int n_batch, long long n_face_total,
                                 int n_face_max, int n_point, int algo,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * Generalised winding number (Jacobson et al. 2013): the sum over the faces of the signed solid
 * angle 2 atan2(det(a,b,c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) over 4 pi, a, b, c the corners minus the point.
 * An integer on a closed, consistently oriented mesh, smooth across holes: the inside test where ray parity is noise.
 *
 * One entry point for both batch forms.  Uniform (vert_offsets == face_offsets == NULL): verts f32 [B,n_vertex,3], faces
 * int64 [n_face_max,3] shared by the batch, n_face_total = B * n_face_max.  Ragged: verts f32 [sum V_b,3] and faces int64
 * [sum F_b,3] (indices local to their shape) back to back, vert_offsets / face_offsets int32 [B+1] (device) their row
 * offsets, n_face_total = sum F_b, n_face_max = max F_b, n_vertex ignored.  points f32 [B,N,3]; winding f32 [B,N].
 * bad_counts (device int32 [4], cleared here): [0] faces with an index outside their mesh, [1] faces with a non-finite
 * corner, [2] non-finite points.  Such faces are never read: every value of their SHAPE is NaN; a non-finite point gets NaN.
 * A mesh without faces gives 0.
 * algo: DEFTET_WN_EXACT = every point against every face in face order; DEFTET_WN_FAST = a centroid octree of depth
 * deftet_winding_number_levels(F_b) per shape, walked by the wave, a node farther than beta radii taken as a dipole, the
 * points sorted by leaf first; DEFTET_WN_FAST_UNSORTED = the same without that sort (same bits; 5-7x slower on incoherent points); DEFTET_WN_AUTO =
 * what deftet_winding_number_resolve_algo(AUTO, n_face_max, n_batch * n_point) returns.  beta: 0 = the default (3), else in [1, 1e6]; the
 * exact path ignores it.  No float atomics; a point's value does not depend on the other points of the call and is the same
 * bits on every run.  n_batch <= 65535.
 * --------------------------------------------------------------------------------- */
#define DEFTET_WN_AUTO 0
#define DEFTET_WN_EXACT 1
#define DEFTET_WN_FAST 2
#define DEFTET_WN_FAST_UNSORTED 3
int deftet_winding_number_levels(int n_face);
int deftet_winding_number_resolve_algo(int algo, int n_face_max, long long n_point_total);
size_t deftet_winding_number_workspace_bytes(int n_batch, long long n_face_total, int n_face_max, int n_point, int algo);
int deftet_winding_number_f32(const float *verts, const int32_t *vert_offsets, const int64_t *faces, const int32_t *face_offsets,
                              const float *points, float *winding, int32_t *bad_counts, int n_batch, int n_vertex,
                              long long n_face_total, int n_face_max, int n_point, int algo, float beta, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * N3  render-side geometry rebuilds of diff_render/diftet_6_subdiv/3_model/
 * prepare_for_wz.py, all on int64 index arrays like the reference's numpy code.  Workspace:
 * deftet_builder_workspace_bytes(n_point, n_tet).  Counts come back in device int32 words.
 *
 * deftet_tet_edges_i64: generate_edge (:184-203) + generate_tet_edge_idx (:223-236).
 *   edges_ex2 int64 [6*n_tet capacity, 2] = unique (min,max) rows in lexicographic order
 *   (np.unique(axis=0)); tet_edge_tx6 int64 [n_tet,6] = row of each tet edge in that list, columns
 *   in the order (0,1),(0,2),(0,3),(1,2),(1,3),(2,3); *bad_flag = 1 if an index is outside [0,n_point).
 * deftet_subdivide_f32: generate_subdivision (:255-301).  points_new f32 [n_point+n_edge,3] and
 *   feat_new f32 [n_point+n_edge,n_feat] = old rows, then edge midpoints (a+b)/2; tet_new int64
 *   [8*n_tet capacity,4]: with subdiv_sig == NULL the eight children of every tet in order, else
 *   the tets with sig == 0 first (unchanged, in order), then the children of those with sig != 0.
 * deftet_point_adj_table_i64: generate_point_adj_idx (:134-146) from the sorted unique ordered pairs
 *   of deftet_tet_point_adj_i32 (A4).  width == 0: adjsum_px1 f32 [n_point] (degrees) and
 *   *max_degree; width > 0: table_pxm int64 [n_point,width] = ascending neighbours, -1 padded.
 *   workspace: (n_point+1) int32.
 * deftet_delete_tet_i64: delete_tet (:171-180): keeps, in order, the tets whose row maximum of
 *   weights_txk f32 [n_tet,k] is > thres (NaN rows are dropped, as np.max propagates NaN).
 * deftet_tet_neighbour_weights_f32: one level of tetweights2tetneighbourweights (3_model/deftet.py:
 *   316-331): out f32 [n_tet,4*k], out[t, j*k+c] = weights[nei[t,j], c], zeros where nei == -1.
 * --------------------------------------------------------------------------------- */
int deftet_tet_edges_i64(const int64_t *tet_tx4, int64_t *edges_ex2, int64_t *tet_edge_tx6, int32_t *n_edge,
                         int32_t *bad_flag, int n_point, int n_tet,
                         void *workspace, size_t workspace_bytes, void *stream);
int deftet_subdivide_f32(const int64_t *tet_tx4, const int64_t *tet_edge_tx6, const int64_t *edges_ex2,
                         const float *points_px3, const float *feat_pxk, const uint8_t *subdiv_sig,
                         float *points_new, float *feat_new, int64_t *tet_new, int32_t *n_tet_new,
                         int n_point, int n_tet, int n_edge, int n_feat,
                         void *workspace, size_t workspace_bytes, void *stream);
int deftet_point_adj_table_i64(const int32_t *pairs_nx2, int n_pairs, int n_point, int64_t *table_pxm, int width,
                               float *adjsum_px1, int32_t *max_degree,
                               void *workspace, size_t workspace_bytes, void *stream);
int deftet_delete_tet_i64(const int64_t *tet_tx4, const float *weights_txk, float thres, int64_t *tet_kept,
                          int32_t *n_kept, int n_tet, int k,
                          void *workspace, size_t workspace_bytes, void *stream);
int deftet_tet_neighbour_weights_f32(const float *weights_txk, const int64_t *nei_tx4, float *out_tx4k,
                                     int n_tet, int k, void *stream);

/* ---------------------------------------------------------------------------------
 * N2  the vertex <-> tet gather either side of the per-tet operators:
 *   tet_bxfx4x3 = torch.gather(vertice_pos, tetrahedron_bxfx4)          layers/DefTet/deftet.py:65-68
 * pos f32 [B,V,3]; tet_idx int64 [idx_batch,T,4] with idx_batch == 1 (one topology shared by all
 * shapes) or == n_batch (the reference's tetrahedron_bxfx4); out f32 [B,T,4,3].
 * An index outside [0,V) (torch.gather raises) yields NaNs and sets *bad_flag (device int32,
 * may be NULL) to 1.
 * Backward: torch's is a scatter-add of 12*T float atomics per shape; here the topology is turned
 * once into a CSR of (tet,corner) incidences per vertex (deftet_tet_vertex_csr_i32: offsets int32
 * [idx_batch*V+1], slots int32 [idx_batch*4*T] holding 4*t+corner in ascending order per vertex;
 * *bad_flag (device int32, required) = 1 when an index is out of range) and
 * deftet_tet_gather_bwd_f32 sums grad_tet f32 [B,T,4,3] per vertex in that order into grad_pos
 * f32 [B,V,3] (overwritten, or added to when accumulate != 0): no atomics, deterministic.
 * --------------------------------------------------------------------------------- */
int deftet_tet_gather_fwd_f32(const float *pos, const int64_t *tet_idx, float *out, int32_t *bad_flag,
                              int n_batch, int n_vertex, int n_tet, int idx_batch, void *stream);
size_t deftet_tet_vertex_csr_workspace_bytes(int idx_batch, int n_vertex, int n_tet);
int deftet_tet_vertex_csr_i32(const int64_t *tet_idx, int32_t *offsets, int32_t *slots, int32_t *bad_flag,
                              int idx_batch, int n_vertex, int n_tet,
                              void *workspace, size_t workspace_bytes, void *stream);
int deftet_tet_gather_bwd_f32(const float *grad_tet, const int32_t *offsets, const int32_t *slots,
                              float *grad_pos, int n_batch, int n_vertex, int n_tet, int idx_batch,
                              int accumulate, void *stream);

/* A1b backward composed with the gather's backward (round 6): the gradient of a caller that owns BOTH the gather
 * (layers/DefTet/deftet.py:65-68) and the query lands on the vertices, grad_pos f32 [B,V,3] (overwritten, or added to when
 * accumulate != 0; the flag also covers grad_pred), without the dense grad_tet [B,T,4,3] of deftet_point_in_tet_bwd_f32 +
 * deftet_tet_gather_bwd_f32: only the rows of tets that accepted a query are written (to `workspace`) and read back.
 * Same arguments as deftet_point_in_tet_bwd_f32 (grad_pts / grad_occ + grad_pred optional) plus the incidence CSR of
 * deftet_tet_vertex_csr_i32.  The result equals the two-call form bit for bit (the same additions in the same order); no
 * floating-point atomics.  Without hit_buf, or beyond two queries per tet, the per-tet lists fill dense rows in the
 * workspace instead (same result). */
size_t deftet_point_in_tet_bwd_to_vertices_workspace_bytes(int n_batch, int n_tet, int n_query);
int deftet_point_in_tet_bwd_to_vertices_f32(const float *tet, const float *pts, const float *cond, const float *grad_w,
                                            const float *grad_occ, const int32_t *hit_buf, const int32_t *csr_offsets,
                                            const int32_t *csr_slots, int idx_batch, float *grad_pos, float *grad_pts,
                                            float *grad_pred, int n_batch, int n_vertex, int n_tet, int n_query,
                                            int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* Indexed input (230): the occupancy query straight from vertex positions and a tet index list.  Corner c of tet t of shape b
 * is pos[b, tet_idx[ib, t, c]], ib = 0 when idx_batch == 1, else b.  pos: f32 [B,V,3], contiguous, 4-byte aligned (a slice of
 * a vertex tensor works); tet_idx: int32 [idx_batch,T,4], contiguous, 16-byte aligned, idx_batch 1 or B.  Every output — cond,
 * bary, occ, hit_buf records, query box — is bit-identical to deftet_point_in_tet_ex_f32 / _scan_ex_f32 /
 * _bwd_to_vertices_f32 run on the tensor deftet_tet_gather_fwd_f32 makes from the same pos and list, for every algo, with and
 * without tet_order and a query box; the records of either forward feed either backward.  An index outside [0, V) reads as a
 * (NaN, NaN, NaN) corner, as in that gather, and sets *bad_flag (device int32, may be NULL) to 1; pos is never read out of
 * range.  Workspaces: deftet_point_in_tet_workspace_bytes and deftet_point_in_tet_bwd_to_vertices_workspace_bytes.
 * The scan form consumes a deftet_point_in_tet_prepare[_ex]_f32 exactly as deftet_point_in_tet_scan_ex_f32 does.  The CSR
 * (deftet_tet_vertex_csr_i32) must be built over the same list, with the same idx_batch. */
int deftet_point_in_tet_indexed_f32(const float *pos, const int32_t *tet_idx, int idx_batch, const float *pts, float *cond,
                                    float *bary, const float *pred, float *occ, int32_t *hit_buf, int n_batch, int n_vertex,
                                    int n_tet, int n_query, int algo, const int32_t *tet_order, const float *query_box_in,
                                    float *query_box_out, int32_t *query_box_misses, int32_t *bad_flag, void *workspace,
                                    size_t workspace_bytes, void *stream);
int deftet_point_in_tet_indexed_scan_f32(const float *pos, const int32_t *tet_idx, int idx_batch, const float *pts, float *cond,
                                         float *bary, const float *pred, float *occ, int32_t *hit_buf, int n_batch, int n_vertex,
                                         int n_tet, int n_query, int algo, const int32_t *tet_order, int32_t *bad_flag,
                                         void *workspace, size_t workspace_bytes, void *stream);
int deftet_point_in_tet_indexed_bwd_to_vertices_f32(const float *pos, const int32_t *tet_idx, int idx_batch, const float *pts,
                                                    const float *cond, const float *grad_w, const float *grad_occ,
                                                    const int32_t *hit_buf, const int32_t *csr_offsets, const int32_t *csr_slots,
                                                    float *grad_pos, float *grad_pts, float *grad_pred, int n_batch, int n_vertex,
                                                    int n_tet, int n_query, int accumulate, void *workspace,
                                                    size_t workspace_bytes, void *stream);

/* A11 fused per-tet energies, layers/DefTet/deftet.py:239-338: out f32 [B,3] =
 * {volume_variance(pow_v), amips_energy(inv_v f32 [T,3,3]; 0 when NULL), edge_length(pow_e)};
 * stats f64 [B,8] is produced by the forward and consumed by the backward, which writes
 * grad_tet f32 [B,T,4,3] = sum_k grad_out[b,k] * d out[b,k] / d tet (fully overwritten). */
size_t deftet_tet_energies_workspace_bytes2(int n_batch, int n_tet); /* what deftet_tet_energies_fwd_f32 needs: + one float per tet */
int deftet_tet_energies_fwd_f32(const float *tet, const float *inv_v, float *out, double *stats, int n_batch, int n_tet,
                                int pow_v, int pow_e, float scale, void *workspace, size_t workspace_bytes, void *stream);
int deftet_tet_energies_bwd_f32(const float *tet, const float *inv_v, const double *stats, const float *grad_out,
                                float *grad_tet, int n_batch, int n_tet, int pow_v, int pow_e, float scale, void *stream);

/* ---------------------------------------------------------------------------------
 * A8  surface-face edge adjacency by position
 * replaces layers/DefTet/tet_face_adj_m_idx/tet_face_adj_m.cpp (forward) ->
 *          tet_face_adj_m_for.cu:72-130.  adj f32 [F,n_max_nei] pre-filled with -1 by the
 * caller (utils.py:47); neighbour g ascending, first n_max_nei kept. */
/* workspace NULL (or n_max_nei > 32): O(F^2) scan; else exact sort-based path, O(F log F). */
size_t deftet_face_edge_adj_workspace_bytes(int n_face);
int deftet_face_edge_adj_f32(const float *face_fx3x3, float *adj_fxm, int n_face, int n_max_nei,
                             void *workspace, size_t workspace_bytes, void *stream);
/* The same operator for a BATCH of surfaces with different face counts — what one training step needs, where the
 * reference loops over the shapes (layers/DefTet/deftet.py:89-103 -> utils/mesh_utils.py:28): face f32 [B,F_max,3,3],
 * adj f32 [B,F_max,n_max_nei] pre-filled with -1; shape b has n_face_host[b] <= F_max faces (HOST integers: the caller
 * built the boundary lists); neighbour indices are local to the shape.  One launch sequence (memset + two kernels)
 * covers the whole batch. */
size_t deftet_face_edge_adj_ragged_workspace_bytes(int n_batch, int n_face_max);
int deftet_face_edge_adj_ragged_f32(const float *face_bxfx3x3, float *adj_bxfxm, int n_batch, int n_face_max,
                                    const int *n_face_host, int n_max_nei, void *workspace, size_t workspace_bytes, void *stream);

/* Normal consistency of B surfaces on their A8 tables: what the reference composes in Python on top of A8
 * (utils/mesh_utils.py:28-39: unit normals n = c / sqrt(|c|^2 + 1e-12), c = (v1 - v0) x (v2 - v0); pairs from the
 * adjacency; mean of 1 - <n_i, n_j>) as one fused launch per direction.  loss f32 [B] = mean over the valid table
 * entries of shape b (0 when there is none); n_face int32 [B] on the DEVICE.  nrm f32 [B,F_max,3] and count f32 [B]
 * are written by the forward for the backward; grad_tri f32 [B,F_max,3,3] is fully overwritten; acc f32 [B,F_max,3]
 * is scratch. */
int deftet_normal_consistency_fwd_f32(const float *tri_bxfx3x3, const float *adj_bxfxm, const int32_t *n_face_dev, float *loss_b,
                                      float *nrm_bxfx3, float *count_b, int n_batch, int n_face_max, int n_max_nei, void *stream);
int deftet_normal_consistency_bwd_f32(const float *tri_bxfx3x3, const float *adj_bxfxm, const int32_t *n_face_dev,
                                      const float *nrm_bxfx3, const float *count_b, const float *grad_loss_b, float *grad_tri,
                                      float *acc_bxfx3, int n_batch, int n_face_max, int n_max_nei, void *stream);

/* ---------------------------------------------------------------------------------
 * Chamfer term of the surface loss (layers/DefTet/deftet.py:174-177 with utils/mesh_utils.py:290-299, :360-374): n_per_face
 * area-uniform samples per predicted face, each measured against its nearest ground-truth point (A10 finds the index).
 *   deftet_face_samples_f32  samples f32 [B, F*K, 3] from tri f32 [B,F,3,3] and uniform numbers r f32 [2,B,F,K]
 *                            (row f*K + j = (1-s) a + s (1-r1) b + s r1 c, s = sqrt(r0): the square-root warp)
 *   deftet_chamfer_fwd_f32   d f32 [B,N] = sqrt(|sample - gt[idx]|^2 + 1e-10) for the first n_valid[b] rows, 0 beyond
 *   deftet_chamfer_bwd_f32   grad_tri f32 [B,F,3,3] for dL/d(sum_rows d)[b] = gscale[b] (one lane per face, no atomics) */
int deftet_face_samples_f32(const float *tri_bxfx3x3, const float *r_2xbxfxk, float *samples_bxnx3, int n_batch, int n_face,
                            int n_per_face, void *stream);
int deftet_chamfer_fwd_f32(const float *samples_bxnx3, const float *gt_bxmx3, const int32_t *idx_bxn, const int32_t *n_valid_b,
                           float *d_bxn, int n_batch, int n_sample, int n_point, void *stream);
int deftet_chamfer_bwd_f32(const float *samples_bxnx3, const float *gt_bxmx3, const int32_t *idx_bxn, const int32_t *n_valid_b,
                           const float *d_bxn, const float *r_2xbxfxk, const float *gscale_b, float *grad_tri_bxfx3x3,
                           int n_batch, int n_face, int n_per_face, int n_point, void *stream);

/* ---------------------------------------------------------------------------------
 * A9  point -> triangle-soup squared distance
 * replaces layers/DefTet/tet_analytic_distance_batch/tet_analytic_distance.cpp ->
 *          tet_analytic_distance_for.cu:256-334 / tet_analytic_distance_back.cu:591-715 */
size_t deftet_tri_dist_workspace_bytes(int n_batch, int n_point, int n_max_face);
/* workspace NULL: streaming scan over all faces; else exact uniform-grid search (same results). */
int deftet_tri_dist_fwd_f32(const float *pts_bxpx3, const float *face_bxfx3x3, const float *n_face_b,
                            float *closest_d, float *closest_f, int n_batch, int n_point, int n_max_face,
                            void *workspace, size_t workspace_bytes, void *stream);
/* The same forward, also handing out the order in which the grid search walked the points of every shape (int32 [B,P],
 * sorted by grid cell; NULL = not wanted; needs a workspace and n_max_face > 0), and the atomic backward that walks the
 * points in that order: neighbouring points share their closest faces, so a wavefront adds their contributions up first
 * and issues one set of atomics per distinct face (same sums up to the order of the fp32 additions). */
int deftet_tri_dist_fwd_order_f32(const float *pts_bxpx3, const float *face_bxfx3x3, const float *n_face_b,
                                  float *closest_d, float *closest_f, int32_t *order_bxp, int n_batch, int n_point,
                                  int n_max_face, void *workspace, size_t workspace_bytes, void *stream);
int deftet_tri_dist_bwd_order_f32(const float *pts_bxpx3, const float *face_bxfx3x3, const float *closest_f,
                                  const float *dl_dclosest_d, const int32_t *order_bxp, float *dldface, int n_batch,
                                  int n_point, int n_face, void *stream);
/* dldface f32 [B,F,3,3] accumulates (zeroed by the wrapper, utils.py:65).  deterministic != 0:
 * contributions are reduced in point order per face instead of by floating-point atomics. */
int deftet_tri_dist_bwd_f32(const float *pts_bxpx3, const float *face_bxfx3x3, const float *closest_f,
                            const float *dl_dclosest_d, float *dldface, int n_batch, int n_point, int n_face,
                            int deterministic, void *stream);

/* ---------------------------------------------------------------------------------
 * A10 brute-force nearest-neighbour index
 * replaces layers/nearest_neighbor/nearest_neighbor.cpp -> nearest_neighbor_cuda.cu:17-80
 * result int32 [B,N]: index of the first point with the strictly smallest fp32 distance. */
size_t deftet_nn_index_workspace_bytes(int n_batch, int n_query, int n_point);
/* workspace NULL: brute-force scan (scalar-stream); else exact uniform-grid shell search. */
int deftet_nn_index_f32(const float *queries_bxnx3, const float *points_bxmx3, int32_t *result_bxn,
                        int n_batch, int n_query, int n_point, void *workspace, size_t workspace_bytes, void *stream);
/* Ragged batch: shape b has n_query_host[b] <= N_max queries (HOST integers; strides stay N_max, rows beyond the count are
 * left untouched) — the samples of predicted surfaces with different face counts.  Like deftet_tri_dist_fwd_f32 and
 * deftet_nn_index_f32 themselves, ONE launch sequence covers (groups of eight shapes of) the batch: every kernel takes
 * the shape from its grid's y/z dimension. */
int deftet_nn_index_ragged_f32(const float *queries_bxnx3, const float *points_bxmx3, int32_t *result_bxn, int n_batch,
                               int n_query_max, int n_point, const int *n_query_host, void *workspace, size_t workspace_bytes,
                               void *stream);

/* ---------------------------------------------------------------------------------
 * Device-wide primitives the operators are built on (deftet_amd/csrc/prims.hpp; nothing in the reference corresponds
 * to them — its CUDA side gets them from Thrust/CUB through torch): a stable LSD radix sort and prefix scans.
 * deftet_radix_sort: ascending, stable, on the low `bits` bits of unsigned 4- or 8-byte keys, optionally carrying 4- or
 * 8-byte values (value_bytes 0 = keys only).  Inputs are not modified, outputs must not alias them.  n_dev (device
 * pointer or NULL): only the first min(n, *n_dev) elements exist — the cost follows that count, not n.
 * deftet_scan: kind 0 exclusive sum, 1 inclusive sum, 2 inclusive running maximum over int32 / int64; in == out allowed. */
size_t deftet_radix_sort_workspace_bytes(long long n, int key_bytes, int value_bytes);
int deftet_radix_sort(const void *keys_in, void *keys_out, const void *values_in, void *values_out, long long n,
                      int key_bytes, int value_bytes, int bits, const int32_t *n_dev, void *workspace,
                      size_t workspace_bytes, void *stream);
size_t deftet_scan_workspace_bytes(long long n, int elem_bytes);
int deftet_scan(const void *in, void *out, long long n, int elem_bytes, int kind, void *workspace, size_t workspace_bytes,
                void *stream);

/* ---------------------------------------------------------------------------------
 * A12 differentiable tet rasterizer with the contract of
 * kaolin.render.mesh.deftet_sparse_render as called at
 * diff_render/diftet_6_subdiv/5_rendereq/deftetrneder.py:97-100 (Kaolin itself is not part
 * of the reference tree: parity unpinned). */
size_t deftet_sparse_render_workspace_bytes(int n_batch, int n_pixel, int n_face, int knum);
/* Which kept faces a pixel RECORDS when more than knum cover it (the output order is always z descending, ties by
 * ascending face index).  Nothing in the reference tree settles this; at its call site knum = 300 against ~60 covering
 * faces, where both give the same images.
 *   NEAREST (default): the knum faces that come first in the output order — what an insertion-sorted list of bounded
 *                      length keeps; independent of how the faces are numbered.
 *   FIRST:             the first knum kept faces in ascending face index (rounds 1-2 of this library). */
#define DEFTET_RASTER_NEAREST 0
#define DEFTET_RASTER_FIRST 1
/* out_w (the barycentric weights of every recorded hit) is optional: NULL skips it.
 * deftet_sparse_render_fwd_f32 = deftet_sparse_render_fwd_policy_f32 with DEFTET_RASTER_NEAREST. */
int deftet_sparse_render_fwd_f32(const float *pixel_bxpx2, const float *range_bxpx2,
                                 const float *face_z_bxfx3, const float *face_xy_bxfx3x2,
                                 const float *face_feat_bxfx3xd, float *out_feat_bxpxkxd,
                                 int64_t *out_face_bxpxk, float *out_w_bxpxkx3,
                                 int n_batch, int n_pixel, int n_face, int n_feat, int knum, float eps,
                                 void *workspace, size_t workspace_bytes, void *stream);
int deftet_sparse_render_fwd_policy_f32(const float *pixel_bxpx2, const float *range_bxpx2,
                                        const float *face_z_bxfx3, const float *face_xy_bxfx3x2,
                                        const float *face_feat_bxfx3xd, float *out_feat_bxpxkxd,
                                        int64_t *out_face_bxpxk, float *out_w_bxpxkx3,
                                        int n_batch, int n_pixel, int n_face, int n_feat, int knum, float eps, int policy,
                                        void *workspace, size_t workspace_bytes, void *stream);
/* backward: gradients to face_vertices_image [B,F,3,2] and face_features [B,F,3,D] (both fully
 * overwritten), none to z / pixels — as Kaolin documents.  Hits are grouped by face with one stable radix
 * sort and reduced by a segmented scan; w_bxpxkx3 is not read (the weights are recomputed from the pixel
 * and the face exactly as the forward computed them) and may be NULL. */
size_t deftet_sparse_render_bwd_workspace_bytes(int n_batch, int n_pixel, int n_face, int knum);
int deftet_sparse_render_bwd_f32(const float *pixel_bxpx2, const float *face_xy_bxfx3x2,
                                 const float *face_feat_bxfx3xd, const int64_t *face_bxpxk,
                                 const float *w_bxpxkx3, const float *grad_out_bxpxkxd,
                                 float *grad_face_xy, float *grad_face_feat,
                                 int n_batch, int n_pixel, int n_face, int n_feat, int knum, float eps,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* Fused rasterize-and-composite (240): the same faces in the same order as deftet_sparse_render_fwd_policy_f32, composited front
 * to back where they are made — alpha_composite (deftet_amd/render/compositing.py) of the layer stack, which is never written.
 * Opacity is feature channel 0, or 1 with depth_channel != 0 (channel 0 is then the layer depth), clamped to [1e-10, 1 - 1e-10];
 * the colour is the remaining D - 1 (D - 2) channels.  Empty slots are zero layers at opacity 1e-10.  Outputs: colour
 * [B,P,Dc] over `background`, coverage [B,P], depth [B,P] over `far_depth` (only with depth_channel; NULL otherwise) and the
 * ranked faces as int32 [B,P,knum] (-1 = empty), which the backward reads.  D >= 2 (>= 3 with depth_channel). */
size_t deftet_sparse_render_composite_workspace_bytes(int n_batch, int n_pixel, int n_face, int n_feat, int knum);
int deftet_sparse_render_composite_fwd_f32(const float *pixel_bxpx2, const float *range_bxpx2,
                                           const float *face_z_bxfx3, const float *face_xy_bxfx3x2,
                                           const float *face_feat_bxfx3xd, int n_batch, int n_pixel, int n_face, int n_feat,
                                           int knum, float eps, int policy, int depth_channel, float background, float far_depth,
                                           float *out_colour_bxpxc, float *out_coverage_bxp, float *out_depth_bxp,
                                           int32_t *out_face_bxpxk, void *workspace, size_t workspace_bytes, void *stream);
/* backward: gradients to face_xy [B,F,3,2] and face_feat [B,F,3,D] (both fully overwritten), none to z.  Any of the three output
 * gradients may be NULL (absent = zero).  No division by 1 - alpha: opacities of exactly 1 are fine. */
size_t deftet_sparse_render_composite_bwd_workspace_bytes(int n_batch, int n_pixel, int n_face, int n_feat, int knum);
int deftet_sparse_render_composite_bwd_f32(const float *pixel_bxpx2, const float *face_xy_bxfx3x2,
                                           const float *face_feat_bxfx3xd, const int32_t *face_bxpxk,
                                           const float *grad_colour_bxpxc, const float *grad_coverage_bxp,
                                           const float *grad_depth_bxp, int n_batch, int n_pixel, int n_face, int n_feat,
                                           int knum, float eps, int depth_channel, float background, float far_depth,
                                           float *grad_face_xy, float *grad_face_feat, void *workspace, size_t workspace_bytes,
                                           void *stream);

/* Vertex Laplacian (250): r = M·x − x over a sparse vertex adjacency M, then r².  Training form: DefTet.laplacian_sparse
 * (layers/DefTet/deftet.py:340-343), M = D⁻¹A, Σ_{i,c} r² per shape.  Render form: Deftet.get_featlap
 * (diff_render/diftet_6_subdiv/3_model/deftet.py:221-241), M = (sum over a padded neighbour table) / w, r² per entry.
 *
 * deftet_vertex_adjacency_csr_i32: nnz (row, col) pairs, int32 or int64 (index_bytes 4 / 8), with optional f32 values (NULL = 1),
 *   to a CSR — offsets int32 [V+1], cols int32 [nnz], vals f32 [nnz] — and its transpose — t_offsets int32 [V+1], t_rows int32
 *   [nnz], t_vals f32 [nnz] (the row of each entry and its value, grouped by column).  vals / t_vals may be NULL (not written).
 *   The entries of a row are ordered by column (DEFTET_VADJ_ROW_COL) or kept in input order (DEFTET_VADJ_ROW_INPUT: a padded
 *   neighbour table read row-major, pads removed); those of a transposed row by row.  Ties keep their input order: duplicate
 *   pairs are kept and summed, as torch.sparse.mm sums an uncoalesced tensor.  An index outside [0, V) sets *bad_flag
 *   (device int32, required, cleared by the call) to 1; such entries are never referenced by the offsets.
 *   Stable radix sorts of this library, no atomics.  Workspace: deftet_vertex_adjacency_workspace_bytes(nnz, V).
 * deftet_vertex_laplacian_fwd_f32: x f32 [B,V,C], 1 <= C <= 16, and the CSR above (nnz entries).
 *   nei = Σ_k vals_k x[cols_k] in CSR order (DEFTET_VLAP_VALUES), or (Σ_k x[cols_k]) / row_weights[i], adds in CSR order then
 *   one IEEE division (DEFTET_VLAP_ROW_DIVISOR; row_weights f32 [V], vals unused).  r = nei − x is written to r f32 [B,V,C];
 *   out f32 [B,V,C] = r² (DEFTET_VLAP_NONE) or out f32 [B] = Σ_{i,c} r² (DEFTET_VLAP_SHAPE, a fixed-order two-stage
 *   reduction through the workspace: deftet_vertex_laplacian_workspace_bytes(B, V); NONE needs none).
 * deftet_vertex_laplacian_bwd_f32: grad_x f32 [B,V,C] (overwritten) = Σ_{i: j ∈ row i} a_ij u_i − u_j, u = 2·g·r, from the
 *   saved r, the upstream gradient grad_out (f32 [B] for SHAPE, [B,V,C] for NONE) and the TRANSPOSED CSR; a_ij = t_vals or
 *   1 / row_weights[i] (applied as a division).  One gather per vertex in transposed-CSR order: no atomics, bit-reproducible.
 * The CSRs must come from deftet_vertex_adjacency_csr_i32 with *bad_flag == 0: the kernels do not re-check their indices. */
#define DEFTET_VADJ_ROW_COL 0
#define DEFTET_VADJ_ROW_INPUT 1
#define DEFTET_VLAP_VALUES 0
#define DEFTET_VLAP_ROW_DIVISOR 1
#define DEFTET_VLAP_NONE 0
#define DEFTET_VLAP_SHAPE 1
size_t deftet_vertex_adjacency_workspace_bytes(int nnz, int n_vertex);
int deftet_vertex_adjacency_csr_i32(const void *row_idx, const void *col_idx, int index_bytes, const float *values, int nnz,
                                    int n_vertex, int order, int32_t *offsets, int32_t *cols, float *vals, int32_t *t_offsets,
                                    int32_t *t_rows, float *t_vals, int32_t *bad_flag, void *workspace, size_t workspace_bytes,
                                    void *stream);
size_t deftet_vertex_laplacian_workspace_bytes(int n_batch, int n_vertex);
int deftet_vertex_laplacian_fwd_f32(const float *x, const int32_t *offsets, const int32_t *cols, const float *vals,
                                    const float *row_weights, int weighting, int reduction, int n_batch, int n_vertex, int n_chan,
                                    int nnz, float *r, float *out, void *workspace, size_t workspace_bytes, void *stream);
int deftet_vertex_laplacian_bwd_f32(const float *r, const float *grad_out, const int32_t *t_offsets, const int32_t *t_rows,
                                    const float *t_vals, const float *row_weights, int weighting, int reduction, int n_batch,
                                    int n_vertex, int n_chan, int nnz, float *grad_x, void *stream);

/* Vertex aggregation (300): out = M·x over the same CSR, for wide rows — the sparse product of the GCN position decoder
 * (GraphConv.forward, layers/gcn_decoder.py:55-56, through sparse_batch_matmul, utils/matrix_utils.py:22-33).
 *
 * deftet_vertex_aggregate_f32: x f32 [B,V,C], any C >= 1; out f32 [B,V,C] (overwritten, must not alias x),
 *   out[b,i,c] = Σ_k vals[k] · x[b, idx[k], c] over k in [offsets[i], offsets[i+1]).  One entry point serves both directions:
 *   the forward passes (offsets, cols, vals), the backward the transposed CSR (t_offsets, t_rows, t_vals) and the upstream
 *   gradient.  Every channel starts at 0.f and takes one fmaf per entry in CSR order, whatever C is: the vector path
 *   (C % 4 == 0 and x, out 16-byte aligned) and the scalar path give the same bits, and a channel's result does not depend
 *   on its neighbours.  No atomics, no workspace, no host synchronisation; nothing is launched when B·V == 0.  B <= 65535.
 *   The CSR must come from deftet_vertex_adjacency_csr_i32 with values and *bad_flag == 0: the kernel does not re-check it. */
int deftet_vertex_aggregate_f32(const float *x, const int32_t *offsets, const int32_t *idx, const float *vals, int n_batch,
                                int n_vertex, int n_channel, int nnz, float *out, void *stream);

/* Evaluation metrics (260): what eval.py:237-260 and utils/point_cloud_utils.py compute with Kaolin, forward only.
 *
 * deftet_point_mesh_distance_f32: points f32 [B,P,3] against face_vertices f32 [B,F,3,3]; n_face (device int32 [B], NULL = F
 *   faces each) limits shape b to its first n_face[b] faces.  dist f32 [B,P] = the squared Euclidean distance to the closest
 *   face, fp32 Ericson (Real-Time Collision Detection §5.1.5) in its branch order; face_idx int64 [B,P] = the first face, in
 *   index order, with the strictly smallest distance; dist_type int32 [B,P]: 0 inside the face, 1/2/3 vertex 0/1/2, 4/5/6 edge
 *   0-1/1-2/2-0.  A zero-area face whose evaluation reaches the interior branch takes the minimum over its three segments; a
 *   face with a non-finite corner never wins; no face gives (+inf, -1, -1); a non-finite point gives (NaN, -1, -1).
 *   The grid search needs deftet_point_mesh_distance_workspace_bytes(B, P, F); _scan_f32 is the streaming scan over every
 *   face with the same evaluation (no workspace).  Both give bit-identical outputs.
 * deftet_sample_points_f32: N points per shape on faces f32 [B,F,3,3] chosen with probability proportional to area (fp32
 *   0.5·|cross(v1−v0, v2−v0)|, or the caller's areas f32 [B,F]) through an exact integer CDF; uniforms f32 [B,N,3] = (u0
 *   face choice, u1, u2 position).  points f32 [B,N,3], face_choice int64 [B,N].  A shape with no faces or zero total area
 *   gets NaN points, face -1 and empty_flag[b] = 1 (device int32 [B], cleared by the call).  Workspace:
 *   deftet_sample_points_workspace_bytes(B, F).
 * deftet_nn_distance_f32: dist f32 [B,N] = A10's distance ((dx·dx + dy·dy) + dz·dz) from query n to points[idx[n]] (idx
 *   int32 [B,N], e.g. from deftet_nn_index_f32), and idx64 (int64 [B,N], optional) = idx.  An index outside [0, M) gives NaN.
 * deftet_surface_metrics_f32: per shape, from the clouds p1 f32 [B,N1,3] (ground truth) and p2 f32 [B,N2,3] (prediction), their
 *   NN indices idx12 int32 [B,N1] (into p2) and idx21 int32 [B,N2] (into p1), and optionally the squared point-to-mesh
 *   distances dist_a f32 [B,Nh] (p1 to the predicted mesh) and dist_b f32 [B,Nh] (p2 to the ground-truth mesh): out f32 [B,5]
 *   = chamfer, chamfer-L1, F-score (radius, extend=True form), mean and max Hausdorff (NaN without dist_a / dist_b).  A
 *   fixed-order two-stage reduction: bit-identical from run to run.  Workspace: deftet_surface_metrics_workspace_bytes(B). */
size_t deftet_point_mesh_distance_workspace_bytes(int n_batch, int n_point, int n_face);
int deftet_point_mesh_distance_f32(const float *points_bxpx3, const float *face_bxfx3x3, const int32_t *n_face_b, int n_batch,
                                   int n_point, int n_face, float *dist_bxp, int64_t *face_idx_bxp, int32_t *dist_type_bxp,
                                   void *workspace, size_t workspace_bytes, void *stream);
int deftet_point_mesh_distance_scan_f32(const float *points_bxpx3, const float *face_bxfx3x3, const int32_t *n_face_b, int n_batch,
                                        int n_point, int n_face, float *dist_bxp, int64_t *face_idx_bxp, int32_t *dist_type_bxp,
                                        void *stream);
size_t deftet_sample_points_workspace_bytes(int n_batch, int n_face);
int deftet_sample_points_f32(const float *face_bxfx3x3, const float *areas_bxf, const int32_t *n_face_b, const float *uniforms_bxnx3,
                             int n_batch, int n_face, int n_sample, float *points_bxnx3, int64_t *face_choice_bxn, int32_t *empty_flag_b,
                             void *workspace, size_t workspace_bytes, void *stream);
int deftet_nn_distance_f32(const float *queries_bxnx3, const float *points_bxmx3, const int32_t *idx_bxn, int n_batch, int n_query,
                           int n_point, float *dist_bxn, int64_t *idx64_bxn, void *stream);
size_t deftet_surface_metrics_workspace_bytes(int n_batch);
int deftet_surface_metrics_f32(const float *p1_bxn1x3, const float *p2_bxn2x3, const int32_t *idx12_bxn1, const int32_t *idx21_bxn2,
                               const float *dist_a_bxnh, const float *dist_b_bxnh, int n_batch, int n1, int n2, int nh, float radius,
                               float *out_bx5, void *workspace, size_t workspace_bytes, void *stream);

/* Rendering straight from the vertices (280): what diff_render/diftet_6_subdiv/3_model/deftet.py:427-468,
 * 3_model/cameraop.py:19-33 and 5_rendereq/deftetrneder.py:78-95 do in torch between the optimiser's per-vertex parameters and
 * the rasterizer's dense per-face buffers.
 *
 * deftet_face_vertex_csr_i32: face_idx int64 [F,3] -> offsets int32 [V+1], slots int32 [3F] holding 3*f+corner in ascending order
 * per vertex; *bad_flag (device int32, required) = 1 when an index is outside [0,V).  The 3-corner twin of
 * deftet_tet_vertex_csr_i32 (the same code).
 *
 * deftet_project_vertices_fwd_f32: pos f32 [pos_batch,V,3], feat f32 [feat_batch,V,D] (each batch 1 = shared by all views, or B),
 * rot f32 [B,3,3], cam_pos f32 [B,3], proj f32 [3] (device) -> z f32 [B,V], xy f32 [B,V,2], act f32 [B,V,Do]:
 *   cam = R (p - c), every row summed left to right;  z = cam.z;  xy = (cam.x proj.x, cam.y proj.y) / (cam.z proj.z) * multiplier;
 *   act = sigmoid(feat), Do = D;  with depth_channel != 0: Do = D + 1, act[...,0] = cam.z (not squashed), act[...,1:] = sigmoid(feat).
 * The operations and their order are those of `perspective`; they are evaluated in fp64 and every output is rounded once (an
 * fp32 chain misses the 1e-5 element-relative bound where cam.x / cam.y cancel).
 * deftet_project_vertices_bwd_f32: g_xy f32 [B,V,2], g_act f32 [B,V,Do] (either may be NULL = zeros) and the forward's INPUTS
 * (recomputing cam in fp64 is cheaper and more exact than reading saved fp32 outputs back) ->
 * grad_pos f32 [pos_batch,V,3], grad_feat f32 [feat_batch,V,D] (either may be NULL = not wanted).  A shared input's gradient is
 * the sum over the views, added in ascending b inside the kernel (in fp64, rounded once).  cam.z gets a gradient through the depth
 * channel only (the rasterizer has none for face_z); cameras get none.
 *
 * deftet_face_gather_fwd_f32: one launch writes face_z f32 [B,F,3], face_xy f32 [B,F,3,2], face_feat f32 [B,F,3,Do] — rows of z,
 * xy, act at face_idx int64 [F,3].  An index outside [0,V) yields NaNs and sets *bad_flag (may be NULL), as
 * deftet_tet_gather_fwd_f32.  xy and face_xy 8-byte aligned.
 * deftet_face_gather_bwd_f32: grad_face_xy f32 [B,F,3,2], grad_face_feat f32 [B,F,3,Do] (either may be NULL = zeros) ->
 * g_xy f32 [B,V,2], g_act f32 [B,V,Do]: every component is the sum over the vertex's incidences, added ONE AFTER THE OTHER in slot
 * order in fp32 (no atomics, no partial sums: the bits do not depend on the launch shape); a vertex without a face gets zeros. */
size_t deftet_face_vertex_csr_workspace_bytes(int n_vertex, int n_face);
int deftet_face_vertex_csr_i32(const int64_t *face_idx, int32_t *offsets, int32_t *slots, int32_t *bad_flag, int n_vertex, int n_face,
                               void *workspace, size_t workspace_bytes, void *stream);
int deftet_project_vertices_fwd_f32(const float *pos, const float *feat, const float *rot, const float *cam_pos, const float *proj,
                                    float multiplier, int depth_channel, float *z, float *xy, float *act, int n_batch, int n_vertex,
                                    int n_feat, int pos_batch, int feat_batch, void *stream);
int deftet_project_vertices_bwd_f32(const float *g_xy, const float *g_act, const float *pos, const float *feat, const float *rot,
                                    const float *cam_pos, const float *proj, float multiplier, int depth_channel, float *grad_pos,
                                    float *grad_feat, int n_batch, int n_vertex, int n_feat, int pos_batch, int feat_batch, void *stream);
int deftet_face_gather_fwd_f32(const float *z, const float *xy, const float *act, const int64_t *face_idx, float *face_z,
                               float *face_xy, float *face_feat, int32_t *bad_flag, int n_batch, int n_vertex, int n_face, int n_act,
                               void *stream);
int deftet_face_gather_bwd_f32(const float *grad_face_xy, const float *grad_face_feat, const int32_t *offsets, const int32_t *slots,
                               float *g_xy, float *g_act, int n_batch, int n_vertex, int n_face, int n_act, void *stream);

/* The point-voxel operators between the point-cloud encoder and the tet grid (pointvoxel.hip).  No float atomics:
 * both scatters are gathers over a stable sort of the points (by voxel, by cell), so every sum has ONE order and two runs agree
 * bit for bit.  deftet_pointvoxel_workspace_bytes(B, N, R) is the size of the one layout the four entries with a workspace carve
 * (the workspace contract at the top).
 *
 * deftet_avg_voxelize_fwd_f32 (vox.cu avg_voxelize): feat f32 [B,C,N], coords i32 [B,3,N] -> out f32 [B,C,R^3], ind i32 [B,N] =
 * x R^2 + y R + z, cnt i32 [B,R^3].  out[b,c,s] = 0 + feat[b,c,i] * (1.0f / (float)cnt[s]) over the points of voxel s in ascending
 * i, every product rounded, then added (the reference kernel with its threads one after another).  A coordinate outside [0,R)
 * gives ind = -1: not counted, no contribution, zero gradient.  N = 0: zeros.
 * deftet_avg_voxelize_bwd_f32: grad_x[b,c,i] = grad_y[b,c,ind[i]] * (1.0f / (float)cnt[ind[i]]), a gather.
 *
 * deftet_voxel_sample_fwd_f32: vol f32 [B,C,R,R,R] read at N points -> out[b, channel_offset + c, p] of out f32 [B,C_total,N] (one
 * call per volume of a list writes its own channel range of the shared result).
 *   pos_mode 0: pos f32 [B,N,3], u = clamp((pos + 0.5) R, 0, R - 1);   pos_mode 1: coords f32 [B,3,N], u = clamp(coords, 0, R - 1)
 *   lo = floor(u), d = u - lo, hi = min(lo + 1, R - 1); weights (1-d | d) as (wx * wy) * wz; corners 000 .. 111, z fastest, index
 *   x R^2 + y R + z; value = the eight products added in that order.  A NaN coordinate is read as 0.
 *   legacy != 0 (trilinear_devox.cu): hi = lo where d == 0; inds i32 [B,8,N] and wgts f32 [B,8,N] (both or neither) are written.
 * deftet_voxel_cells_f32: the sort the volume backward needs, per point set and resolution (shared by volumes of equal R):
 *   perm i32 [B N] (b N + p in cell order, stable), seg i32 [B R^3 + 1] (cell s of shape b owns [seg[b R^3 + s], seg[.. + 1])),
 *   wsorted f32 [8, B N] (the weights in sorted order, corner-major).
 * deftet_voxel_cells_from_inds_i32: the same from recorded inds / wgts [B,8,N], keyed by inds[:,0,:] (outside [0,R^3): dropped);
 *   also isorted i32 [8, B N].
 * deftet_voxel_sample_bwd_vol_f32: two stages, every grad_out element read once.  Per (channel, cell) the eight corner sums
 *   part[k] = sum over the cell's points j in sorted order of wsorted[k][j] * grad_out[b, channel_offset + c, p(j)] (a segment of
 *   up to 32 points one after the other from 0; a longer one by 64 lanes — lane l adds points l, l + 64, ... in that order — and
 *   a fixed butterfly over the lanes, offsets 32 .. 1); then grad_vol[b,c,v] = the up to eight part[k] of the cells v - k, corner
 *   k = 000 .. 111 in that order, from 0.  With isorted a term counts only where isorted[k][j] is the voxel corner k of the cell
 *   nominally lands in (the legacy hi index falls back on lo where its weight is 0): recorded indices that do not have this lo / hi
 *   structure lose their terms, and a non-finite grad_out does not reach voxels through a weight-0 term.  The channels are
 *   chunked so that the partials (32 B R^3 bytes per channel) stay inside the workspace's 64 MiB (one channel if that is larger).
 * deftet_voxel_sample_bwd_pos_f32: grad_pos[b,p,j] (=, or += with accumulate) s * sum_c grad_out[b, channel_offset + c, p] *
 *   d interp / d u_j, channels ascending, s = R for pos_mode 0 and 1 for pos_mode 1 (grad_pos has the layout of pos); 0 for a
 *   coordinate the clamp holds (u <= 0 or u >= R - 1: grid_sample's border rule); the right-hand cell at an interior integer u. */
size_t deftet_pointvoxel_workspace_bytes(int n_batch, int n_point, int resolution);
int deftet_avg_voxelize_fwd_f32(const float *feat, const int32_t *coords, float *out, int32_t *ind, int32_t *cnt, int n_batch,
                                int n_channel, int n_point, int resolution, void *workspace, size_t workspace_bytes, void *stream);
int deftet_avg_voxelize_bwd_f32(const float *grad_y, const int32_t *ind, const int32_t *cnt, float *grad_x, int n_batch, int n_channel,
                                int n_point, int resolution, void *stream);
int deftet_voxel_sample_fwd_f32(const float *vol, const float *pos, float *out, int32_t *inds, float *wgts, int n_batch, int n_channel,
                                int resolution, int n_point, int channel_offset, int n_channel_total, int pos_mode, int legacy,
                                void *stream);
int deftet_voxel_cells_f32(const float *pos, int pos_mode, int32_t *perm, int32_t *seg, float *wsorted, int n_batch, int n_point,
                           int resolution, void *workspace, size_t workspace_bytes, void *stream);
int deftet_voxel_cells_from_inds_i32(const int32_t *inds, const float *wgts, int32_t *perm, int32_t *seg, float *wsorted,
                                     int32_t *isorted, int n_batch, int n_point, int resolution, void *workspace, size_t workspace_bytes,
                                     void *stream);
int deftet_voxel_sample_bwd_vol_f32(const float *grad_out, const int32_t *perm, const int32_t *seg, const float *wsorted,
                                    const int32_t *isorted, float *grad_vol, int n_batch, int n_channel, int resolution, int n_point,
                                    int channel_offset, int n_channel_total, void *workspace, size_t workspace_bytes, void *stream);
int deftet_voxel_sample_bwd_pos_f32(const float *vol, const float *pos, const float *grad_out, float *grad_pos, int n_batch, int n_channel,
                                    int resolution, int n_point, int channel_offset, int n_channel_total, int pos_mode, int accumulate,
                                    void *stream);

/* Pixel-aligned image features (360; image_sample.hip): feature maps read bilinearly at projected points, the
 * operation of DISNDecoder._extract_point_image_features (layers/disn.py:257-305), written with the global feature rows and the
 * appended rows into ONE result out f32 [B, C_total, N], C_total = G + sum C_k + A.  No float atomics; two runs agree bit for bit.
 *
 * map f32 [B,C,H,W]; uv f32 [B,N,2] in grid_sample's convention (uv[..,0] along W, uv[..,1] along H, -1 .. 1 spans the image).
 * border 0: padding "zeros", 1: "border".  In fp32, in this order:
 *   ix = ((x + 1) W - 1) 0.5 (align_corners 0) or (x + 1) 0.5 (W - 1) (align_corners 1), iy likewise with H;
 *   border: ix = fminf(fmaxf(ix, 0), W - 1), iy likewise (a NaN reads pixel 0);
 *   a point with !(ix > -1 && ix < W) or !(iy > -1 && iy < H) is fully outside: value 0, every gradient 0, nothing read and no
 *   float converted to an integer (+-1e30, +-inf, NaN under zeros);
 *   x0 = floor(ix), tx = ix - x0, y likewise; value = the four rounded products added in the order (y0,x0), (y0,x0+1), (y0+1,x0),
 *   (y0+1,x0+1) with weights (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty; a corner outside the map adds 0 and is never read.
 * deftet_image_sample_fwd_f32: out[b, channel_offset + c, p] for the C channels of one map (one call per map of a list); with
 *   global_features f32 [B,G] non-NULL also out[b, g, p] = global_features[b,g], g < n_global, and with append f32 [B,N,A]
 *   non-NULL out[b, C_total - A + a, p] = append[b,p,a].  n_channel = 0 writes those rows only (map may be NULL).
 * deftet_image_cells_f32: the sort the map backward needs, per point set and distinct (H, W, border, align_corners): the key of a
 *   point is b n_cells + (y0 + 1)(W + 1) + (x0 + 1), n_cells = (H + 1)(W + 1) (lo corners from -1: a partially-outside cell has a
 *   key), a fully-outside point sorts behind every cell.  perm i32 [B N] (b N + p in key order, stable), seg i32 [B n_cells + 1],
 *   wsorted f32 [4, B N] (the weights in sorted order, corner-major).
 * deftet_image_sample_bwd_map_f32: grad_map f32 [B,C,H,W] (every element written) in two stages, every grad_out element read
 *   once.  Per (channel, cell) the four corner sums part[k] = sum over the cell's points j in sorted order of wsorted[k][j] *
 *   grad_out[b, channel_offset + c, p(j)] (a segment of up to 32 points one after the other from 0; a longer one by 64 lanes —
 *   lane l adds points l, l + 64, ... in that order — and a fixed butterfly over the lanes, offsets 32 .. 1); then grad_map[b,c,y,x]
 *   = the four part[k] of the cells (y - ky, x - kx), corner k = 2 ky + kx = 0 .. 3 in that order, from 0.  The channels are
 *   chunked so that the partials (16 B n_cells bytes per channel) stay inside the workspace's 32 MiB.
 * deftet_image_sample_bwd_uv_f32: grad_uv[b,p,:] (=, or += with accumulate) (sx gx, sy gy), gx = sum_c grad_out[b, channel_offset
 *   + c, p] * ((v01 - v00)(1 - ty) + (v11 - v10) ty), gy with (v10 - v00)(1 - tx) + (v11 - v01) tx, channels ascending from 0,
 *   texels outside the map counting 0; sx = W / 2 or (W - 1) / 2, sy with H.  0 for a fully-outside point and, under border, for
 *   a coordinate the clamp holds (ix <= 0 or ix >= W - 1, a NaN included); the right-hand cell at an integer ix.
 * deftet_image_sample_bwd_global_f32: grad_global[b,g] = sum_n grad_out[b,g,n] of the first n_global rows of grad_out f32
 *   [B,C_total,N]: one wave per row, lane l adds n = l, l + 64, ... from 0, then the butterfly (offsets 32 .. 1).
 * deftet_image_sample_workspace_bytes(B, N, H, W) is the size of the one layout deftet_image_cells_f32 and
 * deftet_image_sample_bwd_map_f32 carve (the sort's arrays, then the partials; the workspace contract at the top).  The other
 * entries need no workspace. */
size_t deftet_image_sample_workspace_bytes(int n_batch, int n_point, int height, int width);
int deftet_image_sample_fwd_f32(const float *map, const float *uv, const float *global_features, const float *append, float *out,
                                int n_batch, int n_channel, int height, int width, int n_point, int n_global, int n_append,
                                int channel_offset, int n_channel_total, int border, int align_corners, void *stream);
int deftet_image_cells_f32(const float *uv, int32_t *perm, int32_t *seg, float *wsorted, int n_batch, int n_point, int height, int width,
                           int border, int align_corners, void *workspace, size_t workspace_bytes, void *stream);
int deftet_image_sample_bwd_map_f32(const float *grad_out, const int32_t *perm, const int32_t *seg, const float *wsorted, float *grad_map,
                                    int n_batch, int n_channel, int height, int width, int n_point, int channel_offset, int n_channel_total,
                                    void *workspace, size_t workspace_bytes, void *stream);
int deftet_image_sample_bwd_uv_f32(const float *map, const float *uv, const float *grad_out, float *grad_uv, int n_batch, int n_channel,
                                   int height, int width, int n_point, int channel_offset, int n_channel_total, int border,
                                   int align_corners, int accumulate, void *stream);
int deftet_image_sample_bwd_global_f32(const float *grad_out, float *grad_global, int n_batch, int n_global, int n_point, int n_channel_total,
                                       void *stream);

/* Tet-centroid feature sampling (330; tet_centroid_sample.hip): the input of the occupancy decoder,
 * cat(sample_f(mean(gather(pos, tets), 2)[:, chosen], volumes), centroids^T) (layers/pc_model.py:276-306), from the vertices, the
 * tet list and the chosen tets, with nothing of size O(T 4 3) in between.  No float atomics; two runs agree bit for bit.
 *
 * The volume list is three HOST arrays of n_vol <= 8 entries: device pointers vols[k] to f32 [B,C_k,R_k,R_k,R_k], channels[k] = C_k
 * >= 0 and resolutions[k] = R_k >= 1.  pos f32 [B,V,3]; tet_idx i32 [idx_batch,T,4], idx_batch 1 (shared) or B, 16-byte aligned.
 * Slot j < n_slot of every shape is tet select[j] (select i32 [n_slot], shared by the batch, repeats allowed) or, with select NULL,
 * tet first + j (first >= 0, first + n_slot <= T).
 *
 * deftet_tet_centroid_sample_fwd_f32, one launch: cent = (((a + b) + c) + d) * 0.25f per coordinate, corners in list order, every
 *   step rounded (no fused multiply-add with what follows); centroids f32 [B,n_slot,3] receives it, and out f32 [B, sum C_k (+3),
 *   n_slot] receives at rows c_off_k + c what deftet_voxel_sample_fwd_f32 (pos_mode 0, legacy 0) computes at that value, and with
 *   append_pos the value itself in its last three rows.  A tet index outside [0,T) or a vertex index outside [0,V) is not followed:
 *   the slot's centroid and rows are NaN and *bad_flag (optional; the caller zeroes it) is set to 1.
 * The gradient of the volumes is deftet_voxel_cells_f32 (centroids, pos_mode 0) + deftet_voxel_sample_bwd_vol_f32.
 * deftet_tet_centroid_sample_bwd_pos_f32, one launch: grad_cent f32 [B,n_slot,3] = per volume the sum of
 *   deftet_voxel_sample_bwd_pos_f32 (channels ascending from 0, scaled, border rule), the volumes' results added in list order, the
 *   position rows of grad_out (with append_pos) added last: the bits of that chain of calls.  A slot with a NaN centroid gets 0.
 * deftet_tet_centroid_sample_bwd_vertices_f32: grad_pos[b,v,:] (=, or += with accumulate) 0.25f * S, S = one fp32 accumulator from
 *   0 over the incidences of v in the order of the incidence CSR (offsets / slots of deftet_tet_vertex_csr_i32: 4 t + corner
 *   ascending) and, per incidence, over the slots that chose tet t in ascending slot.  Every element of grad_pos is written; a
 *   vertex none of whose tets was chosen gets 0 (or keeps its value with accumulate).  A tet that lists a vertex twice counts
 *   twice, a tet chosen n times counts n times, a select entry outside [0,T) counts nowhere.  With select the slots are grouped
 *   by a stable radix sort in the workspace (deftet_tet_centroid_sample_workspace_bytes(B, T, n_slot)); without
 *   it no workspace is needed. */
size_t deftet_tet_centroid_sample_workspace_bytes(int n_batch, int n_tet, int n_slot);
int deftet_tet_centroid_sample_fwd_f32(const float *const *vols, const int *channels, const int *resolutions, int n_vol, const float *pos,
                                       const int32_t *tet_idx, const int32_t *select, int first, float *out, float *centroids,
                                       int32_t *bad_flag, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_slot, int append_pos,
                                       void *stream);
int deftet_tet_centroid_sample_bwd_pos_f32(const float *const *vols, const int *channels, const int *resolutions, int n_vol,
                                           const float *centroids, const float *grad_out, float *grad_cent, int n_batch, int n_slot,
                                           int append_pos, void *stream);
int deftet_tet_centroid_sample_bwd_vertices_f32(const float *grad_cent, const int32_t *offsets, const int32_t *slots, const int32_t *select,
                                                int first, float *grad_pos, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_slot,
                                                int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* A per-vertex field at query points (340; tet_field_sample.hip): value(p) = sum_k w_k(p) field[vertex k of the
 * tet that holds p], on what the indexed query (deftet_point_in_tet_indexed_f32) returned for the same pos, list and points.
 * No float atomics; two runs agree bit for bit.
 *
 * field f32 [B,V,C], channels last, C >= 1; tet_idx i32 [idx_batch,T,4], idx_batch 1 (shared) or B, 16-byte aligned; cond f32
 * [B,Q,1], -1 = miss; bary f32 [B,Q,4], 16-byte aligned; out, grad_out f32 [B,Q,C].  With t = (int)cond[b,q], ib = 0 when
 * idx_batch == 1, else b, and v_k = tet_idx[ib,t,k]:
 *
 * deftet_tet_field_sample_fwd_f32, one launch: out[b,q,c] = ((w0 f(v0,c) + w1 f(v1,c)) + w2 f(v2,c)) + w3 f(v3,c), every product
 *   and every sum rounded in fp32, in that order (no fused multiply-add).  A miss writes `fill` in every channel.  A vertex index
 *   outside [0,V) (or a cond outside [-1,T)) is not followed: the row is NaN and *bad_flag (optional; the caller zeroes it) is set
 *   to 1.  One lane per query up to C = 8, lanes over the channels of a row beyond.
 * deftet_tet_field_sample_bwd_w_f32, one launch: grad_w[b,q,k] = sum over c ascending of the rounded grad_out[b,q,c] * f(v_k,c),
 *   one fp32 accumulator from 0; a miss and a row the forward refused give 0.  grad_w f32 [B,Q,4] is what
 *   deftet_point_in_tet_indexed_bwd_to_vertices_f32 takes (with the forward's hit records) to grad_pos [B,V,3] and grad_pts.
 * deftet_tet_field_sample_bwd_field_f32: grad_field[b,v,c] (=, or += with accumulate) S, S = one fp32 accumulator from 0 over
 *   the incidences of v in the order of the incidence CSR (offsets / slots of deftet_tet_vertex_csr_i32 over the same list:
 *   4 t + corner ascending) and, per incidence (t, k), over the queries q of shape b with cond == t in ascending q, of the
 *   rounded product bary[b,q,k] * grad_out[b,q,c].  Every element of grad_field is written; a vertex none of whose tets was hit
 *   gets 0 (or keeps its value with accumulate); a tet that lists a vertex twice counts twice.  The per-tet query lists come from
 *   a stable radix sort of the keys b (T + 1) + t (misses at t = T) with the queries as values, in the workspace
 *   (deftet_tet_field_sample_workspace_bytes(B, T, Q)); without a query no workspace is needed.  A vertex runs as long
 *   as the lists of its tets: load skew is accepted. */
size_t deftet_tet_field_sample_workspace_bytes(int n_batch, int n_tet, int n_query);
int deftet_tet_field_sample_fwd_f32(const float *field, const int32_t *tet_idx, const float *cond, const float *bary, float *out,
                                    int32_t *bad_flag, float fill, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_query,
                                    int n_channel, void *stream);
int deftet_tet_field_sample_bwd_w_f32(const float *field, const int32_t *tet_idx, const float *cond, const float *grad_out, float *grad_w,
                                      int n_batch, int n_vertex, int n_tet, int idx_batch, int n_query, int n_channel, void *stream);
int deftet_tet_field_sample_bwd_field_f32(const float *grad_out, const float *cond, const float *bary, const int32_t *offsets,
                                          const int32_t *slots, float *grad_field, int n_batch, int n_vertex, int n_tet, int idx_batch,
                                          int n_query, int n_channel, int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* Ground-truth preparation (310; dataprep.hip): what dataloader.py:24-61 (MakeSurfaceMesh) does with Kaolin's
 * trianglemeshes_to_voxelgrids, extract_odms, project_odms, voxelgrids_to_trianglemeshes and adjacency_matrix.  PARITY UNPINNED:
 * Kaolin's arithmetic cannot be read or run next to this library; the rules below are this library's own.  Forward only.
 * Every output is bit-reproducible (integer atomicOr / atomicAdd only, stable sorts, scans).
 *
 * The bit grid: uint32 [B,R,R,W], W = ceil(R / 32); bit k % 32 of word k / 32 of row (i, j) is voxel (i, j, k); pad bits are 0.
 * 1 <= R <= 1024.
 *
 * deftet_mesh_voxelize_f32: verts f32 [B,V,3], faces i64 [F,3] shared by the batch, origin f32 [B,3] (NULL: the per-shape minimum
 *   of the vertices), scale f32 [B] (NULL: the largest per-shape extent).  q = ((v - origin) / scale) * R in fp32.  Voxel (i,j,k),
 *   the closed box [i,i+1] x [j,j+1] x [k,k+1], is set iff a triangle overlaps it under the 13-axis separating-axis test in fp32
 *   (half size 0.5, corners relative to the voxel centre): the box axes (reject iff min > h or max < -h), the plane n = e0 x e1
 *   (|n.a0| > h (|nx| + |ny| + |nz|)), the nine axes e_i x unit axis (min > r or max < -r, r by the same formula).  Candidates:
 *   i + 1 >= min q_x and i <= max q_x (likewise y, z), clipped to the grid.  Degenerate triangles pass their zero axes; a triangle
 *   with a non-finite corner is skipped; a face index outside [0,V) is skipped and sets stats[2].
 *   bits (required, overwritten) receives the bit grid, vox u8 [B,R,R,R] (optional) its bytes.  stats (device int32 [4], required):
 *   [0] wave tasks, [1] triangles whose candidate box took more than one task (DEFTET_VOXELIZE_UNIT_BUDGET word columns
 *   (i, j, word of k) each), [2] bad index flag, [3] 0.  The task table is int32: n_batch * n_face * ceil(R R W /
 *   DEFTET_VOXELIZE_UNIT_BUDGET), the most tasks the input could have, must be below 2^31 (DEFTET_EINVAL otherwise).
 * deftet_voxel_pack_u8 / _unpack_u8: u8 [B,R,R,R] (non-zero = occupied) <-> the bit grid.
 * deftet_extract_odms_u8: odms i32 [B,6,R,R].  Direction d scans axis d / 2, ascending for even d and descending for odd d; a map
 *   is indexed by the two other axes in ascending axis order; the depth is the number of empty voxels in front of the first
 *   occupied one, R for an empty ray.
 * deftet_project_odms_i32: starts from a full grid (vox_in NULL) or from vox_in; direction d carves the voxels in front of its
 *   depth; out u8 [B,R,R,R] = 1 iff the start voxel is set and fewer than `votes` (1..6) directions carve it.
 * deftet_voxel_fill_b32: out = project(extract(bits)) at votes = 1 on the bit grid, no depth map stored (out must not alias bits).
 * deftet_voxel_surface_count_b32 / _fill_b32: the faces of the occupied region.  Every set voxel and each of its directions
 *   (0 / 1 towards -i / +i, 2 / 3 -j / +j, 4 / 5 -k / +k) whose neighbour is empty or outside emits two triangles wound so that the
 *   normal points out of the voxel: with u, v the axes after the face's axis a (cyclic), corners p00, p10 = p00 + e_u, p11, p01 =
 *   p00 + e_v, the triangles are (p00,p10,p11), (p00,p11,p01) towards +a and (p00,p01,p11), (p00,p11,p10) towards -a.  Rows in
 *   (voxel linear index, direction, triangle) order; vertices are the lattice corners in use, coordinates 0..R as f32, numbered
 *   per shape in ascending (i (R+1) + j) (R+1) + k.  count: offsets i32 [2 (B+1)] = first triangle of every shape and the total,
 *   then first vertex of every shape and the total; it leaves the scanned tables in the workspace, which the fill pass of the
 *   SAME workspace reads: faces i64 [cap_faces,3] (vertex ids local to the shape), verts f32 [cap_verts,3]; rows beyond a
 *   capacity are not written.  The tables are int32: 6 n_batch R R (R + 1), the most triangles a batch could have, must be
 *   below 2^31 (R <= 709 at n_batch = 1; DEFTET_EINVAL otherwise).
 * deftet_face_edges_i32: the unique directed vertex pairs (a, b), a != b, of a triangle list, ascending by (a, b): pairs i32 [6 F,2]
 *   (capacity), n_out i32 [2] = (number of pairs, bad index flag).  Radix sort of the keys a V + b, one entry per run. */
#define DEFTET_VOXELIZE_UNIT_BUDGET 256
size_t deftet_mesh_voxelize_workspace_bytes(int n_batch, int n_face);
int deftet_mesh_voxelize_f32(const float *verts, const int64_t *faces, const float *origin, const float *scale, int n_batch, int n_vertex,
                             int n_face, int resolution, uint32_t *bits, uint8_t *vox, int32_t *stats, void *workspace,
                             size_t workspace_bytes, void *stream);
int deftet_voxel_pack_u8(const uint8_t *vox, int n_batch, int resolution, uint32_t *bits, void *stream);
int deftet_voxel_unpack_u8(const uint32_t *bits, int n_batch, int resolution, uint8_t *vox, void *stream);
int deftet_extract_odms_u8(const uint8_t *vox, int n_batch, int resolution, int32_t *odms, void *stream);
int deftet_project_odms_i32(const int32_t *odms, const uint8_t *vox_in, int n_batch, int resolution, int votes, uint8_t *out, void *stream);
size_t deftet_voxel_fill_workspace_bytes(int n_batch, int resolution);
int deftet_voxel_fill_b32(const uint32_t *bits, int n_batch, int resolution, uint32_t *out, void *workspace, size_t workspace_bytes,
                          void *stream);
size_t deftet_voxel_surface_workspace_bytes(int n_batch, int resolution);
int deftet_voxel_surface_count_b32(const uint32_t *bits, int n_batch, int resolution, int32_t *offsets, void *workspace,
                                   size_t workspace_bytes, void *stream);
int deftet_voxel_surface_fill_b32(const uint32_t *bits, int n_batch, int resolution, long long cap_faces, long long cap_verts, float *verts,
                                  int64_t *faces, void *workspace, size_t workspace_bytes, void *stream);
size_t deftet_face_edges_workspace_bytes(int n_face);
int deftet_face_edges_i32(const int64_t *faces, int n_face, int n_vertex, int32_t *pairs, int32_t *n_out, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * Field gradients on the tets (390; tet_field_grad.hip).  field f32 [B,V,C], pos f32 [B,V,3], tet_idx int32
 * [idx_batch,T,4] (16-byte aligned; idx_batch 1 = one list for every shape, or n_batch), offsets / slots = the incidence CSR of
 * deftet_tet_vertex_csr_i32 for that list.  For a tet with vertices v0..v3 at x0..x3 and e0 = x1 - x0, e1 = x2 - x0, e2 = x3 - x0:
 * n0 = e1 x e2, n1 = e2 x e0, n2 = e0 x e1, det = e0 . n0, vol = det / 6, g_c = (n0 df0 + n1 df1 + n2 df2) / det with
 * df_k = f(v_{k+1},c) - f(v0,c).  A tet is live iff det > 0 in fp32 and its indices lie in [0,V); a dead tet has gradient 0 and
 * volume 0 and takes part in no energy and no backward.  No float atomics: every sum has one order (the file's header), so two
 * runs give the same bits.
 * deftet_tet_field_gradient_fwd_f32: out f32 [B,T,C,3] = g, vol f32 [B,T] (optional).  One launch.  out NULL (field then unused):
 *   the volumes alone.
 * deftet_tet_field_gradient_bwd_f32: grad_out f32 [B,T,C,3] and grad_vol f32 [B,T] (optional) taken to grad_field f32 [B,V,C] and
 *   grad_pos f32 [B,V,3] (each optional, every element written), per vertex one accumulator over its incidences in ascending
 *   4 t + corner.  One launch each; nothing of size O(T) is stored in between.
 * deftet_tet_field_energies_fwd_f32: 1 <= n_channel <= 8 (DEFTET_EINVAL otherwise).  With w_t = vol_t of the live tets and
 *   W = sum w_t: out f32 [B,C,2] = (sum w_t |g_c|^2 / W, sum w_t (|g_c| - target)^2 / W), both 0 when W = 0; the sums in fp64 in
 *   one order.  stats f64 [B,17] = (W, out[:,0] padded to 8, out[:,1] padded to 8) in fp64 is kept by the caller for the backward.
 *   Two launches, g never stored.
 * deftet_tet_field_energies_bwd_f32: grad_out f32 [B,C,2] taken to grad_field and grad_pos (each optional) by the same walk
 *   of the incidence CSR; where |g_c| = 0 the derivative of the second term is taken as 0; all 0 when W = 0.
 * deftet_tet_to_vertex_fwd_f32: values f32 [B,T,C], weights f32 [B,T] (NULL = 1): out f32 [B,V,C] = num / den with
 *   num = sum of fl(w_t values[t,c]) and den = sum of w_t over the vertex's incidences in CSR order, one fp32 accumulator each
 *   from 0, every step rounded; `fill` where den is not > 0.  weight_sum f32 [B,V] (required) receives den.
 * deftet_tet_to_vertex_bwd_f32: grad_values f32 [B,T,C] = w_t * (sum over the corners k = 0..3 of grad_out[v_k,c] /
 *   weight_sum[v_k], one accumulator from 0, a corner whose weight_sum is not > 0 left out).  No gradient on the weights. */
int deftet_tet_field_gradient_fwd_f32(const float *field, const float *pos, const int32_t *tet_idx, float *out, float *vol, int n_batch,
                                      int n_vertex, int n_tet, int idx_batch, int n_channel, void *stream);
int deftet_tet_field_gradient_bwd_f32(const float *grad_out, const float *grad_vol, const float *field, const float *pos,
                                      const int32_t *tet_idx, const int32_t *offsets, const int32_t *slots, float *grad_field,
                                      float *grad_pos, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel, void *stream);
size_t deftet_tet_field_energies_workspace_bytes(int n_batch);
int deftet_tet_field_energies_fwd_f32(const float *field, const float *pos, const int32_t *tet_idx, float *out, double *stats, float target,
                                      int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel, void *workspace,
                                      size_t workspace_bytes, void *stream);
int deftet_tet_field_energies_bwd_f32(const double *stats, const float *grad_out, float target, const float *field, const float *pos,
                                      const int32_t *tet_idx, const int32_t *offsets, const int32_t *slots, float *grad_field,
                                      float *grad_pos, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel, void *stream);
int deftet_tet_to_vertex_fwd_f32(const float *values, const float *weights, const int32_t *offsets, const int32_t *slots, float *out,
                                 float *weight_sum, float fill, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel,
                                 void *stream);
int deftet_tet_to_vertex_bwd_f32(const float *grad_out, const float *weight_sum, const float *weights, const int32_t *tet_idx,
                                 float *grad_values, int n_batch, int n_vertex, int n_tet, int idx_batch, int n_channel, void *stream);

/* ---------------------------------------------------------------------------------
 * Iso-solid measures on the tets (400; tet_iso_measure.hip).  field f32 [B,V], pos, tet_idx, offsets / slots as
 * for the field gradients above; iso a finite f32 (DEFTET_EINVAL otherwise).  A corner is inside iff field > iso (fp32, strict:
 * the predicate of deftet_marching_tets_*).  A tet is live iff it is live to deftet_tet_field_gradient_fwd_f32 (det > 0 in fp32,
 * indices in [0,V)) AND its four corner values are finite; a dead tet has fraction 0, area 0, volume 0 and takes part in no
 * sum and no backward (marching tetrahedra differ here on purpose: there a NaN corner is outside and faces are emitted).
 * Per live tet, in double from the fp32 inputs and rounded once: frac = the share of the tet's volume with field > iso (the
 * field is linear on the tet), area = the area of the iso polygon in the tet; the closed forms stand in the file's header.
 * deftet_tet_iso_fraction_fwd_f32: frac f32 [B,T], area f32 [B,T] (optional), vol f32 [B,T] (optional, the bits of
 *   deftet_tet_field_gradient_fwd_f32's volumes).  One launch.
 * deftet_tet_iso_fraction_bwd_f32: grad_frac, grad_area, grad_vol f32 [B,T] (each optional) taken to grad_field f32 [B,V] and
 *   grad_pos f32 [B,V,3] (each optional, every element written): per vertex one fp64 accumulator per output over its incidences
 *   in ascending 4 t + corner, the tet's case recomputed per incidence, rounded once.  frac does not depend on pos, vol not on
 *   field.  On a kink (a corner on the level) the derivative of the case the predicate picks.  One launch.
 * deftet_tet_iso_measures_fwd_f32: out f32 [B,5] = (sum frac vol, sum area, sum w frac vol, sum w vol, sum vol) over the live
 *   tets, weights w f32 [B,T] (NULL = 1), vol = det / 6 in double; the sums in fp64 in one order, rounded once.  Two launches.
 * deftet_tet_iso_measures_bwd_f32: grad_out f32 [B,5] taken to grad_field and grad_pos by the same walk; the weights are a
 *   constant.  Nothing of size O(T) is stored between forward and backward. */
int deftet_tet_iso_fraction_fwd_f32(const float *field, const float *pos, const int32_t *tet_idx, float *frac, float *area, float *vol,
                                    float iso, int n_batch, int n_vertex, int n_tet, int idx_batch, void *stream);
int deftet_tet_iso_fraction_bwd_f32(const float *grad_frac, const float *grad_area, const float *grad_vol, const float *field,
                                    const float *pos, const int32_t *tet_idx, const int32_t *offsets, const int32_t *slots,
                                    float *grad_field, float *grad_pos, float iso, int n_batch, int n_vertex, int n_tet, int idx_batch,
                                    void *stream);
size_t deftet_tet_iso_measures_workspace_bytes(int n_batch);
int deftet_tet_iso_measures_fwd_f32(const float *field, const float *pos, const int32_t *tet_idx, const float *weights, float *out, float iso,
                                    int n_batch, int n_vertex, int n_tet, int idx_batch, void *workspace, size_t workspace_bytes,
                                    void *stream);
int deftet_tet_iso_measures_bwd_f32(const float *grad_out, const float *weights, const float *field, const float *pos, const int32_t *tet_idx,
                                    const int32_t *offsets, const int32_t *slots, float *grad_field, float *grad_pos, float iso, int n_batch,
                                    int n_vertex, int n_tet, int idx_batch, void *stream);

/* ---------------------------------------------------------------------------------
 * Loop subdivision of triangle surfaces (410; loop_subdivide.hip).  faces int64 [F,3] over V vertices.  An
 * edge with a number of (face, local edge) incidences other than 2 is a crease; a vertex with no crease edge is smooth (kind 0),
 * with exactly two a crease vertex (kind 1), otherwise a corner (kind 2).  The rules and the orders of every fp32 sum stand in
 * the file's header; no float atomics anywhere, so two runs, two batch sizes and two launch shapes give the same bits.
 * deftet_loop_topology_count_i64: sorts the keys min V + max of the 3 F incidences 3 f + k (local edges (f0,f1), (f1,f2), (f2,f0))
 *   and leaves the runs in the workspace for the fill entry.  counts i32 [3] = (n_edge, 1 if an index lies outside [0,V), 1 if a
 *   face names a vertex twice); with shape_offsets i32 [n_shape + 1] (ascending vertex ranges of disjoint shapes; NULL and 0
 *   otherwise) counts has 3 + n_shape + 1 entries, the further ones the first edge id of every shape and n_edge.
 *   n_face > 0, n_vertex > 0, 4 n_face < 2^31 (DEFTET_EINVAL otherwise).
 * deftet_loop_topology_fill_i64: with n_edge as read back (n_vertex + n_edge < 2^31) and the SAME workspace: edges i32 [E,2]
 *   (min,max) ascending, face_edge i32 [F,3], edge_nface i32 [E], edge_opp i32 [E,2] (the opposite corners of the two incidences in
 *   ascending 3 f + k; -1 -1 for a crease), vertex_kind u8 [V], crease_nbr i32 [V,2] (kind 1: the far ends of the two crease
 *   edges in ascending edge id; -1 otherwise), the CSRs of deftet_edge_vertex_csr_i32 over the edges (ev_offsets i32 [V+1],
 *   ev_slots i32 [2E]) and of deftet_face_vertex_csr_i32 over the faces (fv_offsets i32 [V+1], fv_slots i32 [3F]), child_faces
 *   int64 [4F,3]: (a,mab,mca), (b,mbc,mab), (c,mca,mbc), (mab,mbc,mca) with m.. = V + the edge id.
 * deftet_loop_subdivide_fwd_f32: verts f32 [B,V,3], attr f32 [B,V,C] (0 <= C <= 8; NULL with C = 0).  mode 0 = subdivide:
 *   out_verts f32 [B,V+E,3], out_attr f32 [B,V+E,C], rows 0..V-1 the old vertices, row V + e the vertex of edge e; mode 1 =
 *   limit positions: [B,V,..].  One launch, one lane per output row.
 * deftet_loop_subdivide_bwd_f32: the transpose.  grad_out_verts / grad_out_attr (each optional, shaped as the forward's outputs)
 *   taken to grad_verts f32 [B,V,3] / grad_attr f32 [B,V,C] (present exactly where its source is; every element written).  One
 *   launch, one lane per old vertex over both CSRs. */
size_t deftet_loop_topology_workspace_bytes(int n_vertex, int n_face);
int deftet_loop_topology_count_i64(const int64_t *faces, int n_face, int n_vertex, const int32_t *shape_offsets, int n_shape,
                                   int32_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int deftet_loop_topology_fill_i64(const int64_t *faces, int n_face, int n_vertex, int n_edge, int32_t *edges, int32_t *face_edge,
                                  int32_t *edge_nface, int32_t *edge_opp, uint8_t *vertex_kind, int32_t *crease_nbr,
                                  int32_t *ev_offsets, int32_t *ev_slots, int32_t *fv_offsets, int32_t *fv_slots, int64_t *child_faces,
                                  void *workspace, size_t workspace_bytes, void *stream);
int deftet_loop_subdivide_fwd_f32(const float *verts, const float *attr, int n_attr, const int32_t *edges, const int32_t *edge_nface,
                                  const int32_t *edge_opp, const uint8_t *vertex_kind, const int32_t *crease_nbr,
                                  const int32_t *ev_offsets, const int32_t *ev_slots, int n_batch, int n_vertex, int n_edge, int mode,
                                  float *out_verts, float *out_attr, void *stream);
int deftet_loop_subdivide_bwd_f32(const float *grad_out_verts, const float *grad_out_attr, int n_attr, const int32_t *edges,
                                  const int32_t *edge_nface, const int32_t *edge_opp, const uint8_t *vertex_kind,
                                  const int32_t *crease_nbr, const int32_t *ev_offsets, const int32_t *ev_slots,
                                  const int32_t *face_edge, const int32_t *fv_offsets, const int32_t *fv_slots, int n_batch,
                                  int n_vertex, int n_edge, int n_face, int mode, float *grad_verts, float *grad_attr, void *stream);

/* ---------------------------------------------------------------------------------
 * Connected components of a triangle list, their measures and the mesh clean-up (420; mesh_components.hip).
 * faces int64 [F,3] over V vertices; n_shape >= 1 disjoint shapes in one list, face_offsets / vertex_offsets i32 [n_shape + 1]
 * their ascending ranges (one shape: (0, F) and (0, V)).  connectivity 0 = "edge": two faces are connected when they share an
 * undirected vertex pair, whatever the number of faces on it; 1 = "vertex": when they share a vertex.  The label of a
 * component is its smallest face index; every per-component result stands at the label's index and is 0 elsewhere.
 * n_face > 0, n_vertex > 0, 3 n_face < 2^31 (DEFTET_EINVAL otherwise).  Integers wherever integers suffice and no float atomic:
 * the same bits on every run.
 * deftet_mesh_components_i64: labels i32 [F]; n_face, boundary_edges (edges with one incidence), nonmanifold_edges (more than
 *   two), misoriented_edges (two incidences running the same direction) i32 [F]; count i32 [n_shape] components per shape;
 *   with verts f32 [V,3] also area f64 [F] = sum 1/2 |(b-a) x (c-a)| and volume f64 [F] = sum a . (b x c) / 6, in double from the
 *   widened positions, summed in an order that depends on the component's own ascending face list only (chunks of 256 from
 *   the component's start, a fixed tree inside a chunk, the chunk sums in ascending order); area and volume NULL without verts.
 *   flags i32 [3] = (corners outside [0,V), incidences that name one vertex twice, broken union-find chains or exhausted trip
 *   bounds); such corners are never followed.
 * deftet_mesh_cleanup_count_i64: the same, then on the device in this order: drop_voids drops every closed component (its
 *   three edge counts 0) with volume < 0; min_faces = m > 0 drops components with fewer faces; min_area = a > 0 those with
 *   area < a; keep_largest keeps per shape the survivor with the most faces (largest_by 0) or the largest area (1), the smaller
 *   label among equals.  drop_voids, min_area and largest_by 1 need verts.  counts i32 [3 + 2 (n_shape + 1)]: the flags, then the
 *   kept faces before every shape and their total, then the kept vertices (those a kept face references) likewise — the one
 *   read-back.  The scans stay in the workspace for the fill entry.
 * deftet_mesh_cleanup_fill_i64: with the totals as read back and the SAME workspace: faces_out int64 [F',3] in ascending old
 *   index, numbered from its shape's first kept vertex; vertex_map int64 [V'] and face_map int64 [F'], the old indices, ascending.
 * deftet_mesh_gather_fwd_f32: out_verts[r] = verts[vertex_map[r]], out_attr[r] = attr[vertex_map[r]] (0 <= C <= 8; NULL with
 *   C = 0); one launch.  deftet_mesh_gather_bwd_f32: the transpose for an injective ascending map — grad rows copied to the kept
 *   vertices, zeros everywhere else, every element written; each output present exactly where its source is; one launch. */
size_t deftet_mesh_components_workspace_bytes(int n_vertex, int n_face, int n_shape);
int deftet_mesh_components_i64(const int64_t *faces, int n_face, int n_vertex, const float *verts, const int32_t *face_offsets, int n_shape,
                               int connectivity, int32_t *labels, int32_t *n_face_out, int32_t *boundary_edges,
                               int32_t *nonmanifold_edges, int32_t *misoriented_edges, double *area, double *volume, int32_t *count,
                               int32_t *flags, void *workspace, size_t workspace_bytes, void *stream);
int deftet_mesh_cleanup_count_i64(const int64_t *faces, int n_face, int n_vertex, const float *verts, const int32_t *face_offsets,
                                  const int32_t *vertex_offsets, int n_shape, int connectivity, int keep_largest, int min_faces,
                                  double min_area, int drop_voids, int largest_by, int32_t *labels, int32_t *n_face_out,
                                  int32_t *boundary_edges, int32_t *nonmanifold_edges, int32_t *misoriented_edges, double *area,
                                  double *volume, int32_t *count, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int deftet_mesh_cleanup_fill_i64(const int64_t *faces, int n_face, int n_vertex, const int32_t *face_offsets, const int32_t *vertex_offsets,
                                 int n_shape, long long n_face_out, long long n_vertex_out, int64_t *faces_out, int64_t *vertex_map,
                                 int64_t *face_map, void *workspace, size_t workspace_bytes, void *stream);
int deftet_mesh_gather_fwd_f32(const float *verts, const float *attr, int n_attr, const int64_t *vertex_map, int n_vertex, int n_vertex_out,
                               float *out_verts, float *out_attr, void *stream);
int deftet_mesh_gather_bwd_f32(const float *grad_out_verts, const float *grad_out_attr, int n_attr, const int64_t *vertex_map, int n_vertex,
                               int n_vertex_out, float *grad_verts, float *grad_attr, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DEFTET_HIP_H_ */
