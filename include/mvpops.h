/*
 * mvpops.h -- C ABI of libmvpops.so, the MI355X (gfx950) point-cloud op layer.
 *
 * This is the native drop-in boundary for the MVP_Benchmark hot path.  The
 * reference reaches its CUDA kernels through 8 pybind11 modules whose bodies
 * immediately unwrap at::Tensor into raw pointers + int sizes + a stream and
 * call a `*_kernel_launcher` (e.g. utils/mm3d_pn2/ops/ball_query/src/
 * ball_query.cpp:30-43).  Each entry point below replaces one of those
 * launchers / pybind functions; the reference interface it replaces is cited
 * as path:line relative to the reference tree.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer (hipMalloc / torch CUDA tensor
 *     data_ptr) to a contiguous row-major array; float = IEEE binary32,
 *     int = int32.  No torch types cross this boundary.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *     Launches are asynchronous on that stream; nothing here synchronises.
 *   - the caller owns every buffer, including scratch; the library allocates
 *     nothing and keeps no DATA between calls (re-entrant, any thread).  The one
 *     piece of process-wide state is the set of tuning knobs behind
 *     mvp_emd_configure (which kernels mvp_emd_forward launches, never what it
 *     computes); nothing else is remembered.
 *   - return value: MVP_OK (0) on success; MVP_EBADSHAPE / MVP_EBADARG for
 *     argument errors (nothing launched); MVP_ELAUNCH if HIP reported a
 *     launch error (details via mvp_last_hip_error()).  The reference's
 *     `printf + return code that Python ignores` / `exit(-1)` behaviour
 *     (chamfer3D.cu:145-152, furthest_point_sample_cuda.cu:204-208) becomes
 *     a return code the host side turns into an exception.
 *   - initial contents required of output/scratch buffers are stated per
 *     function; they are exactly what the reference's Python wrappers
 *     establish before calling into native code.
 */
#ifndef MVPOPS_H_
#define MVPOPS_H_

#ifdef __cplusplus
extern "C" {
#endif

#define MVP_OK 0
#define MVP_EBADSHAPE (-1)
#define MVP_EBADARG (-2)
#define MVP_ELAUNCH (-3)

/* ABI version of this header; bumped on any signature change. */
#define MVP_ABI_VERSION 25
int mvp_abi_version(void);

/* hipGetErrorString of the last launch failure seen on the calling thread
 * ("" if none). */
const char *mvp_last_hip_error(void);

/* ---------------------------------------------------------------- Chamfer */

/* Replaces chamfer_3D.forward = chamfer_forward
 * (utils/metrics/CD/chamfer3D/chamfer_cuda.cpp:17-19,31) ->
 * chamfer_cuda_forward (chamfer3D.cu:136-154) -> NmDistanceKernel x2
 * (chamfer3D.cu:12-134).
 * xyz1 (b,n,3), xyz2 (b,m,3) -> dist1 (b,n), idx1 (b,n): squared distance to
 * and index of the nearest point of xyz2; dist2/idx2 (b,m): roles swapped.
 * Ties: lowest index wins.  Outputs are fully overwritten (n,m >= 1).
 * Non-finite input (this entry point and mvp_chamfer_forward_sorted, bit for
 * bit the same): a candidate whose computed distance is NaN is never the
 * nearest.  +inf is a value like any other (lowest index among the candidates
 * at the minimum).  A query for which every distance is NaN gets dist = NaN
 * (quiet, positive: 0x7fc00000) and idx = 0.  Every index is in [0, m)
 * whatever the input.  The reference agrees on a NaN query; for a NaN
 * *candidate* its result depends on the candidate's place in a 512-tile and is
 * not reproduced. */
int mvp_chamfer_forward(int b, int n, int m, const float *xyz1,
                        const float *xyz2, float *dist1, float *dist2,
                        int *idx1, int *idx2, void *stream);

/* Same contract and bit-identical results as mvp_chamfer_forward, for large
 * clouds: both sides are first bucketed into Morton-ordered cells inside the
 * caller's scratch (mvp_chamfer_scratch_bytes(b,n,m) bytes, 16-byte aligned,
 * contents irrelevant), then candidate tiles whose bounding box is farther
 * than the current best of a whole wave of queries are skipped.  Falls back
 * to the exhaustive kernel (scratch unused, may be NULL) when n or m < 2048
 * or n*m < 2^24. */
long long mvp_chamfer_scratch_bytes(int b, int n, int m);
int mvp_chamfer_forward_sorted(int b, int n, int m, const float *xyz1,
                               const float *xyz2, float *dist1, float *dist2,
                               int *idx1, int *idx2, void *scratch,
                               long long scratch_bytes, void *stream);

/* Replaces chamfer_3D.backward = chamfer_backward (chamfer_cuda.cpp:22-27,32)
 * -> chamfer_cuda_backward (chamfer3D.cu:176-195) -> NmDistanceGradKernel x2
 * (chamfer3D.cu:155-174).
 * gradxyz1 (b,n,3) and gradxyz2 (b,m,3) are ACCUMULATED into (float atomics)
 * and must be zero on entry (dist_chamfer_3D.py:56-57). */
int mvp_chamfer_backward(int b, int n, int m, const float *xyz1,
                         const float *xyz2, float *gradxyz1, float *gradxyz2,
                         const float *graddist1, const float *graddist2,
                         const int *idx1, const int *idx2, void *stream);

/* -------------------------------------------------------------------- EMD */

/* Bytes of device scratch mvp_emd_forward needs for (b, n); the reference
 * passes 11 scratch tensors instead (utils/metrics/EMD/emd_module.py:54-65).
 * Contents on entry are irrelevant (the kernel initialises its own state).
 * The last 16*b bytes of the buffer passed to mvp_emd_forward (its
 * scratch_bytes, a multiple of 16) receive per-cloud {int64 rounds, int64 bids}
 * statistics. */
long long mvp_emd_scratch_bytes(int b, int n);

/* Replaces emd.forward = emd_forward (utils/metrics/EMD/emd.cpp:14-20,29) ->
 * emd_cuda_forward (emd_cuda.cu:228-282): `iters` auction rounds of
 * {clear, calc_unass_cnt, calc_unass_cnt_sum, calc_unass_idx, Bid, GetMax,
 * Assign} (emd_cuda.cu:23-215) then CalcDist (:217-226), with the initial
 * state of emd_module.py:54-65.
 * xyz1 = prediction (b,n,3), xyz2 = ground truth (b,n,3) ->
 * dist (b,n) squared matched distance, assignment (b,n) index into xyz2
 * (may be non-injective after the forced last round).
 * Guards as emd_cuda.cu:236-249: n %% 1024 == 0, b <= 512 (-> MVP_EBADSHAPE);
 * iters >= 1; eps > 0 (-> MVP_EBADARG: the auction needs strictly positive bid
 * increments, and the search prunes on prices that never fall).  Deterministic: GetMax's racy last-writer (emd_cuda.cu:188-191)
 * is pinned to the highest qualifying bidder index.
 * Launches: one small memset (barrier words, hand-over records, statistics),
 * then a persistent cooperative kernel in which up to 8 workgroups share a
 * cloud when b leaves CUs free (b*W <= CU count), and -- for auctions of more
 * than 64 rounds, unless mvp_emd_configure(split = 0) -- a second cooperative
 * kernel of the same shape (csrc/emd_lean.hip) that takes a cloud over for the
 * rounds in which every workgroup has fewer bidders than four per wave (from
 * round ~100 on at 16384 points); it exits at once for clouds the first kernel
 * finished.  With split >= 2, 33..64 clouds of at least 4096 points on
 * four workgroups each, that second kernel stops before round 300 and a third launch runs the
 * rest with the workgroups dealt out again: the clouds with the most persons
 * still unassigned -- the ones whose rounds cost most -- get 8, the lightest 2
 * (64 uniform clouds: 8,5,4,4,3,3,3,2 over the eight clouds of an XCD; equally
 * loaded clouds keep 4 each)
 * (csrc/emd_lean.hip, emd_lean_tiers_kernel).  With split >= 4 (3: in a launch of its own)
 * clouds of at most 4096 points leave the clustered kernels as soon as at most
 * `resident_cap` (16) persons are unassigned -- round ~300 of 3000 at 1024
 * points, 500-850 at 2048, 900-1700 at 4096 -- and member 0 of the cloud's cluster
 * (csrc/emd_resident.h, one workgroup per cloud) runs the remaining rounds
 * with the whole auction state in that workgroup's LDS: no global memory access
 * inside a round.  With split = 5 (the default) the clustered kernels switch to
 * gathered-bid rounds once at most 256 persons of a cloud (of <= 16384 points)
 * are unassigned: a bid is published as a tagged 16-byte record, every workgroup
 * of the cluster settles every bid on its own view of the cloud (owner map in
 * LDS) and a round has one cluster-wide wait instead of a bid atomic and two
 * all-gathers (csrc/emd_lean.hip).  Once at most 16 persons of a cloud of more than
 * 4096 (and at most 16384) points are unassigned -- most of the 3000 rounds when the
 * prediction is near its ground truth -- member 0 of the cluster finishes the
 * auction alone: a wave per bidder with its record in registers, the round's bids and
 * the owner map in LDS, one barrier between Bid and Assign
 * (csrc/emd_lean_round_few.inc).  Which workgroups serve a cloud, in which
 * launch and in which kind of round, never changes a bit of the result.
 * If a cluster wait is abandoned (members not co-resident for tens of seconds;
 * never seen) dist is filled with NaN, assignment with -1 and the statistics
 * word `rounds` is negative: the host wrapper checks for NaN lazily, and
 * mvp_emd_backward skips negative indices. */
int mvp_emd_forward(int b, int n, const float *xyz1, const float *xyz2,
                    float *dist, int *assignment, float eps, int iters,
                    void *scratch, long long scratch_bytes, void *stream);

/* Tuning / A-B knobs of mvp_emd_forward, process-wide (compiled-in defaults; the release
 * library reads NOTHING from the environment -- the MVP_EMD_* variables of rounds 1-4 exist
 * only in libmvpops_hooks.so, the same sources built with -DMVP_TEST_HOOKS for the tests and
 * A/B tools).  A negative argument leaves that knob unchanged.
 *   cluster     0 = automatic, or 1|2|4|8: cap of the workgroups per cloud
 *   same_xcd    0: keep write-through stores even when a cluster shares an XCD
 *   split       5 (default): as 4, with gathered-bid rounds once <= 256 persons are unassigned;
 *               4: as 2, and clouds of <= 4096 points finish LDS-resident
 *               (csrc/emd_resident.h) on member 0 of their cluster, inside the second kernel's launch;
 *               3: the same in a launch of its own (every cloud waits for the last to get there); 2: the tail rounds run in the second kernel, from
 *               round 300 on with cluster widths by load (8 .. 2 workgroups);
 *               1: second kernel, fixed widths; 0: the first kernel runs every round
 *   resident_cap  1..64 (default 16: one wave of the workgroup per unassigned person; more: several per wave): unassigned persons at which a cloud of <= 4096
 *               points moves into LDS (split >= 3)
 * This is the library's only process-wide state (kept under a mutex; a call of
 * mvp_emd_forward reads one consistent copy).  Results never depend on it
 * (every setting is bit-identical: tests/test_gpu_ops.py).  A caller that must not
 * share state (several devices / threads with different plans) passes the plan on
 * the call instead: mvp_emd_forward_plan below. */
int mvp_emd_configure(int cluster, int same_xcd, int split, int resident_cap);

/* mvp_emd_forward with its launch plan on the call (ABI 17): the fields mean what
 * mvp_emd_configure's arguments mean; a NULL plan or a negative field selects the
 * compiled-in default.  Neither reads nor writes the process-wide knobs.  Same
 * results bit for bit. */
typedef struct MvpEmdPlan {
  int cluster, same_xcd, split, resident_cap;
} MvpEmdPlan;
int mvp_emd_forward_plan(int b, int n, const float *xyz1, const float *xyz2,
                         float *dist, int *assignment, float eps, int iters,
                         void *scratch, long long scratch_bytes,
                         const MvpEmdPlan *plan, void *stream);

/* Replaces emd.backward = emd_backward (emd.cpp:22-25,30) ->
 * emd_cuda_backward (emd_cuda.cu:302-316) -> NmDistanceGradKernel (:284-300).
 * gradxyz (b,n,3) accumulated into; must be zero on entry
 * (emd_module.py:77). */
int mvp_emd_backward(int b, int n, const float *xyz1, const float *xyz2,
                     float *gradxyz, const float *graddist, const int *idx,
                     void *stream);

/* -------------------------------------------------- furthest point sample */

/* Replaces furthest_point_sample_ext.furthest_point_sampling_wrapper
 * (utils/mm3d_pn2/ops/furthest_point_sample/src/furthest_point_sample.cpp:
 * 32-43,61) -> furthest_point_sampling_kernel_launcher
 * (src/furthest_point_sample_cuda.cu:143-209).
 * points (b,n,3); temp (b,n) scratch (the reference requires it pre-filled
 * with 1e10, furthest_point_sample.py:30; this implementation does not read
 * it on entry but leaves the final min-distances in it); idx (b,m) out.
 * Tie order is the reference's: strided first-strict-max per thread then the
 * shared-memory tree of furthest_point_sample_cuda.cu:17-23. */
int mvp_furthest_point_sampling(int b, int n, int m, const float *points,
                                float *temp, int *idx, void *stream);

/* Same contract and index-identical results as mvp_furthest_point_sampling for
 * 4096 < n <= 16384 (elsewhere it simply forwards to it): the cloud is first
 * Morton-sorted into the caller's scratch (mvp_fps_scratch_bytes(b,n) bytes,
 * 16-byte aligned, contents irrelevant) so that a lane owns a compact run of
 * points and whole waves skip the distance update when the new sample cannot
 * lower any of their running minima. */
long long mvp_fps_scratch_bytes(int b, int n);
int mvp_furthest_point_sampling_sorted(int b, int n, int m, const float *points,
                                       float *temp, int *idx, void *scratch,
                                       long long scratch_bytes, void *stream);

/* Replaces furthest_point_sampling_with_dist_wrapper
 * (furthest_point_sample.cpp:45-58,63) -> ..._with_dist_kernel_launcher
 * (furthest_point_sample_cuda.cu:333-400).  points_dist (b,n,n). */
int mvp_furthest_point_sampling_with_dist(int b, int n, int m,
                                          const float *points_dist,
                                          float *temp, int *idx, void *stream);

/* The same sampling (same indices, same temp) with w = 2 or 4 workgroups per cloud: a lane owns
 * 1/w of the points the reference's thread scans, the members exchange their local winners
 * through memory once per round (csrc/fps.hip: fps_cluster_kernel).  n a multiple of w * 1024,
 * n <= 16384; scratch of mvp_fps_cluster_scratch_bytes(b) bytes.  MVP_EBADSHAPE when the shape is
 * not covered or the cooperative launch does not fit the device (the caller then uses
 * mvp_furthest_point_sampling).  Opt-in: measured slower or on par, see profiles/NOTES_r1-r3_design_notebook.md section 10. */
long long mvp_fps_cluster_scratch_bytes(int b);
int mvp_furthest_point_sampling_cluster(int b, int n, int m, int w, const float *points,
                                        float *temp, int *idx, void *scratch,
                                        long long scratch_bytes, void *stream);


/* ---------------------------------------------------- ball_query/knn/3nn */

/* Replaces ball_query_ext.ball_query_wrapper
 * (utils/mm3d_pn2/ops/ball_query/src/ball_query.cpp:30-43,46) ->
 * ball_query_kernel_launcher (src/ball_query_cuda.cu:56-78).
 * new_xyz (b,m,3) centres, xyz (b,n,3) -> idx (b,m,nsample).  Rows with no
 * hit keep the zeros the caller put there (ball_query.py:35); this
 * implementation writes every slot itself, so idx need not be pre-zeroed.
 * Non-finite input: a distance that is NaN is no hit, so a centre with a NaN
 * coordinate gets a row of zeros and points with a NaN coordinate are skipped. */
int mvp_ball_query(int b, int n, int m, float min_radius, float max_radius,
                   int nsample, const float *new_xyz, const float *xyz,
                   int *idx, void *stream);

/* Replaces knn_ext.knn_wrapper (utils/mm3d_pn2/ops/knn/src/knn.cpp:28-41,45)
 * -> knn_kernel_launcher (src/knn_cuda.cu:97-115).
 * xyz (b,n,3), new_xyz (b,m,3) -> idx (b,m,nsample), dist2 (b,m,nsample),
 * ascending; 1 <= nsample <= 100.  Slot order follows the reference's
 * max-heap + heap-sort (knn_cuda.cu:26-53).
 * As in the reference the heap starts at (1e10, 0) and admits by strict `<`:
 * a distance that is NaN, +inf or >= 1e10 is never admitted, and a query with
 * fewer than nsample admissible candidates keeps (1e10, 0) in the slots left
 * (last, the list being ascending).  Every index is in [0, n). */
int mvp_knn(int b, int n, int m, int nsample, const float *xyz,
            const float *new_xyz, int *idx, float *dist2, void *stream);

/* The same result as mvp_knn for large clouds without the exhaustive scan: both point sets are
 * Morton-sorted into caller scratch (mvp_knn_scratch_bytes(b, n, m) bytes, 16-byte aligned, contents
 * irrelevant) and every query searches outwards through boxed tiles, keeping k + 1 candidates; queries
 * whose k + 1 smallest distances are not pairwise different (lattices, duplicates: there the reference's
 * result depends on its sequence of heap operations, knn_cuda.cu:26-53,80-90) are recomputed by the
 * exhaustive kernel.  n < 4096, m < 1024 or nsample > 32: forwards to mvp_knn.  Non-finite input: equal to
 * mvp_knn on the same input (such queries end with equal 1e10 slots and take the recomputation). */
long long mvp_knn_scratch_bytes(int b, int n, int m);
int mvp_knn_sorted(int b, int n, int m, int nsample, const float *xyz,
                   const float *new_xyz, int *idx, float *dist2, void *scratch,
                   long long scratch_bytes, void *stream);

/* Feature-space neighbour search of the models (no native counterpart in the
 * reference: completion/model_utils.py:242-247 builds `-xx - inner - xx^T` on a
 * materialised (B,N,N) matrix and calls torch.topk).  dot (b,n,n) = x^T x from a
 * library GEMM, sq (b,n) = |x_i|^2 -> idx (b,n,k): per row i the k largest of
 * val[i][j] = fl(fl(-sq[j] - fl(-2 dot[i][j])) - sq[i]), sorted descending (self
 * first); equal to torch.topk's indices wherever the values are distinct.  k <= n.
 *  - k <= 64 and n <= 16384 (one wave per row streaming the matrix): exactly the
 *    top k by (value descending, column ascending) -- among equal values the lower
 *    columns are chosen and come first, at the cut too, and -0 == +0.  The result
 *    does not depend on n % 4 or on the alignment of `dot` (which only pick the
 *    load width).  Columns whose value is NaN or -inf are never chosen: a row
 *    with fewer than k others lists those first, in order, and fills the rest of
 *    its slots with column 0, so every index is in [0, n).
 *  - otherwise (n > 16384) the tile kernel, k <= 47 (MVP_EBADSHAPE beyond): the k
 *    largest values in descending order at k distinct columns (NaN and -inf as
 *    above); which of several columns of equal value is taken, and their order,
 *    is unspecified, so the indices are pinned only where a value differs from
 *    its neighbours. */
int mvp_topk_gram(int b, int n, int k, const float *dot, const float *sq,
                  int *idx, void *stream);

/* Replaces interpolate_ext.three_nn_wrapper
 * (utils/mm3d_pn2/ops/interpolate/src/interpolate.cpp:46-56,88) ->
 * three_nn_kernel_launcher (src/three_nn_cuda.cu:67-89).
 * unknown (b,n,3), known (b,m,3) -> dist2 (b,n,3) SQUARED, idx (b,n,3).
 * The three bests start at (+inf, 0) and are replaced by strict `<`: a distance
 * that is NaN or +inf is never selected, and with fewer than three others the
 * slots left keep (+inf, 0). */
int mvp_three_nn(int b, int n, int m, const float *unknown,
                 const float *known, float *dist2, int *idx, void *stream);

/* ----------------------------------------- interpolate / gather / group */

/* Replaces interpolate_ext.three_interpolate_wrapper (interpolate.cpp:58-70,
 * 89) -> three_interpolate_kernel_launcher
 * (src/three_interpolate_cuda.cu:37-59).
 * points (b,c,m), idx (b,n,3), weight (b,n,3) -> out (b,c,n). */
int mvp_three_interpolate(int b, int c, int m, int n, const float *points,
                          const int *idx, const float *weight, float *out,
                          void *stream);

/* Replaces interpolate_ext.three_interpolate_grad_wrapper
 * (interpolate.cpp:72-85,91) -> three_interpolate_grad_kernel_launcher
 * (three_interpolate_cuda.cu:86-108).  grad_points (b,c,m) accumulated into;
 * zero on entry (three_interpolate.py:53). */
int mvp_three_interpolate_grad(int b, int c, int n, int m,
                               const float *grad_out, const int *idx,
                               const float *weight, float *grad_points,
                               void *stream);

/* Replaces gather_points_ext.gather_points_wrapper
 * (utils/mm3d_pn2/ops/gather_points/src/gather_points.cpp:28-38,55) ->
 * gather_points_kernel_launcher (src/gather_points_cuda.cu:28-49).
 * points (b,c,n), idx (b,npoints) -> out (b,c,npoints). */
int mvp_gather_points(int b, int c, int n, int npoints, const float *points,
                      const int *idx, float *out, void *stream);

/* Gather + max over the k neighbours of every output point, fused (not an operator of the
 * reference: it replaces the gather_points + torch.max pair of edge_preserve_sampling,
 * completion/model_utils.py:101-104, without materialising the (b,c,npoints,k) neighbour tensor):
 *   out[b,c,p] = max_j points[b,c, idx[b,p,j]],  arg[b,c,p] = idx[b,p,j*] for the FIRST maximal j.
 * points (b,c,n), idx (b,npoints,k) int32 in [0,n), out (b,c,npoints), arg (b,c,npoints) int32.
 * MVP_EBADSHAPE when a row of n floats does not fit the 96 KiB LDS staging buffer (n > 24576): the
 * caller then gathers and reduces. */
int mvp_gather_max(int b, int c, int n, int npoints, int k, const float *points,
                   const int *idx, float *out, int *arg, void *stream);

/* Its gradient: grad_points[b,c, arg[b,c,p]] += grad_out[b,c,p] (overwrite != 0: every element of
 * grad_points is written, no zero fill by the caller). */
int mvp_gather_max_grad(int b, int c, int n, int npoints, const float *grad_out,
                        const int *arg, float *grad_points, int overwrite, void *stream);

/* Replaces gather_points_ext.gather_points_grad_wrapper
 * (gather_points.cpp:40-52,57) -> gather_points_grad_kernel_launcher
 * (gather_points_cuda.cu:72-94).  grad_points (b,c,n) accumulated into; zero
 * on entry (gather_points.py:44). */
int mvp_gather_points_grad(int b, int c, int n, int npoints,
                           const float *grad_out, const int *idx,
                           float *grad_points, void *stream);

/* Replaces group_points_ext.forward
 * (utils/mm3d_pn2/ops/group_points/src/group_points.cpp:45-57,60) ->
 * group_points_kernel_launcher (src/group_points_cuda.cu:81-101).
 * points (b,c,n), idx (b,npoints,nsample) -> out (b,c,npoints,nsample). */
int mvp_group_points(int b, int c, int n, int npoints, int nsample,
                     const float *points, const int *idx, float *out,
                     void *stream);

/* Replaces group_points_ext.backward (group_points.cpp:31-43,61) ->
 * group_points_grad_kernel_launcher (group_points_cuda.cu:33-54).
 * grad_points (b,c,n) accumulated into; zero on entry
 * (group_points.py:213). */
int mvp_group_points_grad(int b, int c, int n, int npoints, int nsample,
                          const float *grad_out, const int *idx,
                          float *grad_points, void *stream);

/* ---- the three scatter-add gradients with caller-provided scratch.
 * Same contracts as mvp_gather_points_grad / mvp_group_points_grad /
 * mvp_three_interpolate_grad (same reference launchers; grad_points is
 * accumulated into).  The index array is inverted once per call into `scratch`
 * (counting sort by destination per cloud and chunk of grad_out columns), then
 * every destination is summed by one thread from LDS-staged grad_out columns:
 * no float atomics, grad_out read once.  mvp_scatter_scratch_bytes(b, n_dst,
 * m_src, r): bytes needed for b clouds, n_dst destination points (the n of
 * gather/group, the m of three_interpolate), m_src grad_out columns (npoints,
 * npoints*nsample, or three_interpolate's n) and r index entries per column
 * (1, or 3 for three_interpolate); 0 = shape not covered (n_dst > 8192).  With
 * scratch == NULL, scratch_bytes too small or a shape that is not covered the
 * _ws entry points run the plain ones.
 * mode: bit 0 MVP_SCATTER_OVERWRITE -- grad_points is WRITTEN (every element;
 * it need not be zero on entry and is not read), saving the caller's zero fill
 * and the read-modify-write; bit 1 MVP_SCATTER_INDEX_READY -- `scratch` still
 * holds the inverted index a previous call built for exactly this idx (and
 * weight): the sort is skipped (the same neighbour graph is differentiated
 * through several gathers per step). */
#define MVP_SCATTER_OVERWRITE 1
#define MVP_SCATTER_INDEX_READY 2
long long mvp_scatter_scratch_bytes(int b, int n_dst, int m_src, int r);
int mvp_gather_points_grad_ws(int b, int c, int n, int npoints,
                              const float *grad_out, const int *idx,
                              float *grad_points, void *scratch,
                              long long scratch_bytes, int mode, void *stream);
int mvp_group_points_grad_ws(int b, int c, int n, int npoints, int nsample,
                             const float *grad_out, const int *idx,
                             float *grad_points, void *scratch,
                             long long scratch_bytes, int mode, void *stream);
int mvp_three_interpolate_grad_ws(int b, int c, int n, int m,
                                  const float *grad_out, const int *idx,
                                  const float *weight, float *grad_points,
                                  void *scratch, long long scratch_bytes,
                                  int mode, void *stream);

/* Shared-weight neighbourhood aggregation of VRCNet's point self-attention (no
 * native counterpart in the reference: completion/models/vrcnet.py:52-55
 * materialises w.repeat(1, share, 1, 1), the product and its sum over k).
 * w (b,cw,k,n), v (b,share*cw,k,n) -> out (b,share*cw,n):
 *   out[b, s*cw+m, n] = sum_k w[b,m,k,n] * v[b, s*cw+m, k, n]   (k ascending).
 * share in {1,2,4,8,16} (MVP_EBADSHAPE otherwise). */
int mvp_share_weighted_sum(int b, int share, int cw, int k, int n,
                           const float *w, const float *v, float *out,
                           void *stream);
/* Its gradients in one pass: grad_v (b,share*cw,k,n) = w * grad_out (broadcast
 * over k), grad_w (b,cw,k,n) = sum_s grad_out[b,s*cw+m,n] * v[b,s*cw+m,k,n];
 * both overwritten. */
int mvp_share_weighted_sum_grad(int b, int share, int cw, int k, int n,
                                const float *w, const float *v,
                                const float *grad_out, float *grad_w,
                                float *grad_v, void *stream);

/* Weight (and bias) gradient of a per-point / per-edge linear map -- a 1x1
 * convolution y = W x + bias on x (b,cin,len), len = N or k*N positions per
 * cloud -- for few output channels (the models' Conv1d/Conv2d(kernel_size=1)
 * layers of completion/models; the reference leaves them to cuDNN):
 *   gw[co][ci] = sum_{b,l} gy[b][co][l] * x[b][ci][l]   (overwritten)
 *   gb[co]     = sum_{b,l} gy[b][co][l]                 (overwritten; gb may be NULL)
 * cout <= 64, len % 4 == 0, x and gy 16-byte aligned.  scratch:
 * mvp_pointwise_wgrad_scratch_bytes(b, cin, cout, len) bytes of per-workgroup
 * partial sums (0 = shape not covered), added up in a fixed order. */
long long mvp_pointwise_wgrad_scratch_bytes(int b, int cin, int cout, int len);
int mvp_pointwise_wgrad(int b, int cin, int cout, int len, const float *x,
                        const float *gy, float *gw, float *gb, void *scratch,
                        long long scratch_bytes, void *stream);

/* Data gradient of the same layers:  gx[b][ci][l] = sum_co weight[co][ci] * gy[b][co][l]
 * (overwritten); cin, cout <= 64, len % 4 == 0, gy and gx 16-byte aligned.  The callers'
 * ReLU mask is applied to gy beforehand (mvp_benchmark_amd/pointwise.py). */
int mvp_pointwise_dgrad(int b, int cin, int cout, int len, const float *weight,
                        const float *gy, float *gx, void *stream);

/* The same aggregation with the gather of the neighbours' values fused in:
 *   out[b, s*cw + m, p] = sum_k w[b, m, k, p] * v[b, s*cw + m, idx[b, k, p]]
 * w (b,cw,k,n), v (b,share*cw,n_src) the per-point values, idx (b,k,n) int32 the neighbour lists (k-major);
 * the (b, share*cw, k, n) tensor of gathered values (vrcnet.py:45-55 builds it with get_edge_features) is never
 * formed.  share * n_src * 4 <= 96 KiB (mvp_share_gather_sum_lds_bytes); bit-identical to mvp_group_points +
 * mvp_share_weighted_sum.  _grad: grad_w (b,cw,k,n) and grad_vals (b,share*cw,k,n) = the gradient of the gathered
 * values, to be scattered into grad_v by mvp_group_points_grad(_ws). */
long long mvp_share_gather_sum_lds_bytes(int share, int n_src);
int mvp_share_gather_sum(int b, int share, int cw, int k, int n_src, int n, const float *w,
                         const float *v, const int *idx, float *out, void *stream);
int mvp_share_gather_sum_grad(int b, int share, int cw, int k, int n_src, int n, const float *w,
                              const float *v, const int *idx, const float *grad_out,
                              float *grad_w, float *grad_vals, void *stream);

/* Dense edge convolution of ECG (completion/models/ecg.py:36-65, Dense_conv: conv / ReLU / cat / max over the k
 * neighbours, op by op on (B, ., N, k) tensors; no native counterpart in the reference) with the per-edge values kept
 * in registers.  layers = dense_n - 1 stack layers (0..2), g in {8,16,24,32}, 1 <= k <= 64, n <= 65536; anything else
 * is MVP_EBADSHAPE.  Per cloud, point p, neighbour slot j:
 *   edge[:, j] = relu(a[:, p] + nb[idx[j, p], :])
 *   y_i[:, j]  = act_i(W_i [edge; y_1; ..; y_{i-1}][:, j] + ctr_i[:, p])   act_i = ReLU for i < layers, none for the last
 *   out[:, p]  = [max_j edge, max_j y_1, .., max_j y_layers],  arg = the FIRST maximal j per channel (mvp_gather_max's rule)
 * a (b,g,n), ctr (b,layers*g,n), idx (b,k,n) int32 k-major (clamped into [0,n)), out and arg (b,(layers+1)*g,n) are
 * channel-major.  nb (b,n,g) is POINT-major and 16-byte aligned: a neighbour's g values are one contiguous read.
 * w: layer i (1-based) is (g, i*g) row-major over [edge, y_1 .. y_{i-1}], layers back to back, g*g*layers*(layers+1)/2
 * floats.  Every y is an fma chain over ascending input channels started from the centre term.  With layers == 0,
 * ctr, w, grad_ctr, grad_w and scratch may be NULL.  Non-finite inputs: unspecified.
 * _grad recomputes the per-edge values from the inputs and arg and writes (never accumulates into) grad_a (b,g,n),
 * grad_ctr (b,layers*g,n), grad_w and -- unless grad_edge is NULL -- grad_edge (b,g,k,n), the gradient at the pre-ReLU
 * edge sum, to be scattered into grad_nb (b,g,n) by mvp_group_points_grad(_ws); grad_a is its sum over k.  grad_w: one
 * partial sum per workgroup of 64 points in `scratch` (mvp_dense_edge_conv_scratch_bytes: 4 * b * ceil(n/64) * the
 * floats of w bytes, at least 4; 0 = shape not covered), added up in a fixed order by a second launch: no float
 * atomics, the same bits on every run. */
long long mvp_dense_edge_conv_scratch_bytes(int b, int g, int layers, int k, int n);
int mvp_dense_edge_conv(int b, int g, int layers, int k, int n, const float *a, const float *nb,
                        const int *idx, const float *ctr, const float *w, float *out, int *arg,
                        void *stream);
int mvp_dense_edge_conv_grad(int b, int g, int layers, int k, int n, const float *a, const float *nb,
                             const int *idx, const float *ctr, const float *w, const int *arg,
                             const float *grad_out, float *grad_a, float *grad_edge, float *grad_ctr,
                             float *grad_w, void *scratch, long long scratch_bytes, void *stream);

/* ABI 22.  DGCNN's edge MLP in inference (registration/models/dcp.py: DGCNN; the reference, dcp.py:286-318, runs conv /
 * BatchNorm / ReLU / max op by op on (B, C, N, k) tensors): the neighbourhood gather, `stages` 1x1 convolutions each
 * followed by a per-channel affine map (BatchNorm with its running statistics) and ReLU, and the max over the k
 * neighbours after every stage, in one kernel -- no (b, C, k, n) tensor exists in global memory.  Per cloud, point p,
 * slot j:
 *   e_0[:, j] = [x[:, idx[j, p]] ; x[:, p]]                        (neighbour first, then centre)
 *   e_i[:, j] = relu(scale_i * (W_i e_{i-1}[:, j]) + shift_i)      i = 1 .. stages
 *   out[off_i : off_i + w_i, p] = max_j e_i[:, j]                  off_i = w_1 + .. + w_{i-1}
 * x (b,c,n), idx (b,k,n) int32 k-major (the knn operator's layout; values in [0,n), clamped into it), w: W_1 (w1, 2c),
 * W_2 (w2, w1), .. row-major, packed back to back, 16-byte aligned; scale, shift (w1 + .. + w_stages); out
 * (b, w1 + .. + w_stages, n), fully overwritten.
 * Shapes: stages 1..4 with the unused widths 0, every used width a multiple of 32 in [32, 256], c 1..4, k 1..64,
 * b <= 65535, n * k < 2^31; anything else is MVP_EBADSHAPE (before the null checks); b == 0 or n == 0 does nothing.
 * Arithmetic: W_1 e_0 is an fmaf chain over ascending input channels on the vector ALU, W_i e_{i-1} for i >= 2 runs on
 * v_mfma_f32_32x32x2_f32 (float32 in, float32 accumulate, a k-ordered fmaf chain); the affine map is one fmaf.
 * Non-finite values, as mvp_pointwise_mfma: relu(t) is the select t < 0 ? 0 : t (a NaN stays a NaN), the maximum is NaN
 * if a member is (torch.max).  No scratch, no atomics: the same bits on every run.  Forward only. */
int mvp_edge_mlp_max(int b, int c, int n, int k, int stages, int w1, int w2, int w3, int w4,
                     const float *x, const int *idx, const float *w, const float *scale,
                     const float *shift, float *out, void *stream);

/* ABI 25.  Multi-head attention of DCP's transformer in inference (registration/models/dcp.py: MultiHeadedAttention; the
 * reference, dcp.py:26-33, 210-229, runs q k^T, the division by sqrt(d), the softmax, the second product and a transposed copy as
 * five steps over a (b, h, nq, nk) score tensor) as one kernel.  Per (cloud, head t, query row i):
 *   s_ij = scale * <q_i, k_j>,      out_i = sum_j softmax_j(s_ij) v_j
 * q and out are (b, nq, h d), k and v (b, nk, h d), contiguous float32, head t in the columns t d .. t d + d of a row: the
 * layout the module's nn.Linear projections write and read, no head transpose or reshape copy exists on this route.
 * Covered: d in {32, 64, 96, 128}; any nq, nk >= 1 (partial tiles on both axes); b, h >= 1; every tensor below 2^31
 * elements; all four pointers on 16-byte addresses.  b == 0 or nq == 0 launches nothing and returns MVP_OK; anything
 * else outside the coverage (a negative size, h < 1, nk == 0, another d, a NULL or misaligned pointer) is MVP_EBADARG,
 * with nothing launched and no output written.
 * Arithmetic: flash-style, tiles of 32 keys with an online softmax (running maximum and sum per query); both products run
 * on v_mfma_f32_32x32x2_f32 (float32 in, float32 accumulate, a k-ordered fmaf chain); the weights are
 * exp2((s_ij - m) log2 e) with the hardware's exp2, out = O / l in IEEE division.  No score or weight is written to global
 * memory; no scratch, no atomics: every output is a fixed expression, the same bits on every run, and a row's bits do not
 * depend on which other query rows are in the call.
 * Non-finite values: the maximum masks nothing, so a NaN in query row i makes output row i NaN in that head's columns and
 * no other row; a NaN in key j, or in a column of value j, makes every row of that (cloud, head) NaN (value: in that
 * column); no other (cloud, head) is touched.  +-inf inputs are not specified.  Forward only. */
int mvp_attention_forward(int b, int h, int nq, int nk, int d, const float *q, const float *k, const float *v,
                          float scale, float *out, void *stream);

/* ------------------------------------------- grouped-feature MLP on MFMA */

/* 1x1 convolution / per-point linear map with a fused epilogue, on the matrix
 * cores (v_mfma_f32_32x32x2_f32: float32 in, float32 accumulate -- the result is
 * a k-ordered fmaf chain, no reduced precision).  No native counterpart in the
 * reference, which calls cuDNN through nn.Conv1d / nn.Conv2d(kernel_size=1) and
 * separate bias / ReLU / add / max kernels (completion/model_utils.py:26-55,
 * completion/models/vrcnet.py:21-57, ecg.py:36-65, pcn.py).
 *   x (b, cin, len), w (cout, cin) [w_kmajor = 0] or (cin, cout) [w_kmajor = 1],
 *         its rows ldw floats apart (0 = dense; a (cout, cin) weight with cin % 4 != 0
 *         is read with 16-byte loads when the caller pads its rows to ldw % 4 == 0)
 *   xmask (b, cin, len) or NULL: x is taken as 0 where xmask <= 0 (the data
 *         gradient of a fused ReLU: x = grad_out, xmask = the layer's output);
 *         aten.threshold_backward's select -- an Inf of x is dropped there, not
 *         multiplied, and x passes where xmask is NaN
 *   t[b,co,l] = sum_ci w(co,ci) x[b,ci,l] + bias[co]        (bias may be NULL)
 *   t = t < 0 ? 0 : t  (torch.relu: a NaN stays a NaN)      if relu
 *   u[b,co,g] = max_{l in group g} t[b,co,l]                groups of `group`
 *                                                            consecutive columns
 *                                                            (1, 2, 4, ..., 32);
 *                                                            NaN if a member is
 *                                                            (torch.max)
 *   y[b,co,g] = u + residual[b,co,g]                        (residual may be NULL)
 * y, residual: (b, cout, len / group).  len % 4 == 0, len % group == 0, x 16-byte
 * aligned.  The data gradient of the plain map is the same call with the forward
 * weight, cin and cout swapped and w_kmajor = 1. */
int mvp_pointwise_mfma(int b, int cin, int cout, int len, const float *x,
                       const float *xmask, const float *w, int ldw, int w_kmajor,
                       const float *bias, const float *residual, int relu,
                       int group, float *y, void *stream);

/* ABI 18.  The same map with the activation / residual patterns of the relational encoder in the GEMM's
 * prologue and epilogue, so that `conv(relu(x))`, `relu(conv(a) + x)`, `relu(conv(f) + g[b])` and two
 * convolutions of one input cost no elementwise pass and no copy (completion/models/vrcnet.py:34-36,54-57
 * pre-activation ReLUs of SA_module; :151,172 and :255-296 residual sums followed by ReLU; :283-285 conv6 over
 * cat(global feature tiled, features); :160,172 conv1 / conv_res of one input).  mvp_pointwise_mfma is this call
 * with bias_per_cloud = 0, flags = relu ? MVP_PW_RELU : 0, m_split = 0.
 *   flags  MVP_PW_X_RELU       x counts as relu(x) (on load; x itself is not written)
 *          MVP_PW_RELU         t = relu(t) before the group maximum and the residual (mvp_pointwise_mfma's relu)
 *          MVP_PW_RES_IS_MASK  `residual` is a mask: y = residual <= 0 ? 0 : u instead of u + residual -- the data
 *                              gradient of conv(relu(x)): aten.threshold_backward(W^T grad_out, x, 0)
 *          MVP_PW_RELU_AFTER   y = relu(y) after the residual / mask
 *          Non-finite values: relu(t) is the select t < 0 ? 0 : t, so a NaN stays a NaN as under torch.relu (never
 *          fmaxf, which would answer 0); the masks (xmask, gymask, RES_IS_MASK) are threshold_backward's select, so u
 *          passes where the mask is NaN and an Inf of u is dropped where the mask is <= 0; the group maximum is NaN if a
 *          member is (torch.max).  These are what autograd of the float32 PyTorch composition yields on every route.
 *   bias_per_cloud != 0: bias is (b, cout) -- the share of a per-cloud vector in a convolution over
 *          cat(vector tiled over the positions, features) -- instead of (cout)
 *   m_split (0, or a multiple of 32 below cout; then residual == NULL, group == 1, y2 != NULL): output rows below
 *          m_split go to y (b, m_split, len), the others to y2 (b, cout - m_split, len).
 * Arithmetic: the same k-ordered fmaf chain per output as mvp_pointwise_mfma; every fused step is the exact
 * float operation the separate pass would perform (add, select), non-finite inputs included. */
#define MVP_PW_RELU 1
#define MVP_PW_RELU_AFTER 2
#define MVP_PW_RES_IS_MASK 4
#define MVP_PW_X_RELU 8
int mvp_pointwise_mfma_ex(int b, int cin, int cout, int len, const float *x,
                          const float *xmask, const float *w, int ldw, int w_kmajor,
                          const float *bias, int bias_per_cloud, const float *residual,
                          int flags, int group, float *y, int m_split, float *y2,
                          void *stream);

/* ABI 20.  mvp_pointwise_mfma_ex (group = 1, one output) with the reduction split over workgroups: for a long reduction
 * whose output has too few tiles to fill the chip (ECG's bottleneck layers, ecg.py: 1864 -> 768 at 256 points, 2824 /
 * 1800 -> 1024 at 64 points).  Two launches: every workgroup reduces one chunk [s k_chunk, min((s + 1) k_chunk, cin)) of one
 * output tile (x masked / rectified on load as in the plain call) and writes its raw accumulators to
 * scratch[s][b][cout][len]; a second kernel adds the chunks and applies the epilogue.  No atomics: bit-reproducible.
 *   mvp_pointwise_mfma_splitk_plan           the suggested k_chunk (a multiple of 16), or 0 = do not split.  Host-only and
 *          pure (no GPU needed).  cin is the reduction length, cout the output rows: the data gradient asks with the two
 *          swapped, as it calls.  Splits only cin > 512 with fewer than 512 output tiles (128 x 128; 64 rows for
 *          cout <= 64, 64 columns for len <= 64): min(ceil(512 / tiles), cin / 128, 16) chunks, if that is >= 2.
 *   mvp_pointwise_mfma_splitk_scratch_bytes  ceil(cin / k_chunk) * b * cout * len * 4, or 0 where the call would refuse the
 *          shape or the chunk.
 *   mvp_pointwise_mfma_splitk                the arguments of mvp_pointwise_mfma_ex without group, m_split and y2.
 *          k_chunk not a positive multiple of 16: MVP_EBADARG; more than 32 chunks: MVP_EBADSHAPE; scratch NULL, not
 *          16-byte aligned or smaller than the query's answer: MVP_EBADARG; every shape, flag and alignment refusal of
 *          mvp_pointwise_mfma_ex unchanged.  k_chunk >= cin (one chunk) IS mvp_pointwise_mfma_ex; scratch may be NULL then.
 * Arithmetic: chunk s is what mvp_pointwise_mfma_ex yields on the K-slice [s k_chunk, ...) of x (xmask) and w with the
 * same prologue, no bias and no epilogue flags, bit for bit (a chunk is a whole number of the kernel's 16-wide slabs, so
 * the order of every matrix instruction coincides); y is ((p0 + p1) + p2) + ... followed by + bias, ReLU, + residual (or
 * the residual as a mask), ReLU as the flags say, each one IEEE float32 operation with the non-finite contract above. */
int mvp_pointwise_mfma_splitk_plan(int b, int cin, int cout, int len);
long long mvp_pointwise_mfma_splitk_scratch_bytes(int b, int cin, int cout, int len, int k_chunk);
int mvp_pointwise_mfma_splitk(int b, int cin, int cout, int len, const float *x,
                              const float *xmask, const float *w, int ldw, int w_kmajor,
                              const float *bias, int bias_per_cloud, const float *residual,
                              int flags, float *y, int k_chunk, void *scratch,
                              long long scratch_bytes, void *stream);

/* ABI 16.  (W x + bias) [then ReLU], reduced with max over ALL positions of a cloud inside the GEMM's epilogue
 * -- the PointNet stage of the completion networks: `x = self.conv4(x); global_feature, _ = torch.max(x, 2)`
 * (completion/models/pcn.py:29-30; vrcnet.py:281-282 conv5; ecg.py:137-138 gf_conv) -- without writing the
 * (b, cout, len) tensor: val (b, cout) = the maxima, idx (b, cout) int32 = the first position that attains each
 * (what torch.max reports; the sparse backward pass mvp_pointwise_max_backward takes it).  Arithmetic as
 * mvp_pointwise_mfma: val equals its output reduced with max, bit for bit; a NaN in a row (of either sign, with or without
 * the ReLU) makes val NaN and idx the first NaN, as torch.max reports.  keys: b * cout * 8 bytes of caller
 * scratch, 8-byte aligned, contents irrelevant.  w (cout, cin) row-major with row stride ldw (0 = cin). */
int mvp_pointwise_mfma_max(int b, int cin, int cout, int len, const float *x, const float *w, int ldw,
                           const float *bias, int relu, float *val, int *idx, void *keys, long long keys_bytes,
                           void *stream);

/* Weight (and bias) gradient of the same map on the matrix cores:
 *   gw[co,ci] = sum_b sum_l g[b,co,l] x[b,ci,l],  gb[co] = sum_b sum_l g[b,co,l]
 * with g = gy, or 0 where gymask <= 0 and gy elsewhere (fused ReLU: aten.threshold_backward's
 * select, so gy passes where gymask is NaN).  gb may be
 * NULL.  The b*len positions are split over workgroups that write partial
 * tiles into `scratch` (mvp_pointwise_wgrad_mfma_scratch_bytes(...) bytes; 0 =
 * shape not covered), a second kernel adds them in a fixed order: no float
 * atomics, bit-reproducible.  gw, gb are overwritten.  len % 4 == 0, operands
 * 16-byte aligned. */
long long mvp_pointwise_wgrad_mfma_scratch_bytes(int b, int cin, int cout,
                                                 int len, int with_bias);
int mvp_pointwise_wgrad_mfma(int b, int cin, int cout, int len, const float *x,
                             const float *gy, const float *gymask, float *gw,
                             float *gb, void *scratch, long long scratch_bytes,
                             void *stream);
/* ABI 18.  x_relu != 0: x counts as relu(x) (NaN stays NaN) on load -- the weight gradient of conv(relu(x)) from the
 * tensor the layer was handed, not from a stored relu(x). */
int mvp_pointwise_wgrad_mfma_ex(int b, int cin, int cout, int len, const float *x, int x_relu,
                                const float *gy, const float *gymask, float *gw,
                                float *gb, void *scratch, long long scratch_bytes,
                                void *stream);

/* Backward pass of a 1x1 convolution followed by a max over the positions,
 * v[b][co] = max_l (W x + bias)[b][co][l] (the PointNet stage: completion/models/pcn.py:25-31,
 * conv5 of vrcnet.py's relational encoder, ecg.py's gf_conv), through the b * cout winning
 * positions only:
 *   gw[co][ci]   = sum_b g[b][co] x[b][ci][idx[b][co]],   gb[co] = sum_b g[b][co]
 *   gx[b][ci][l] = sum_{co : idx[b][co] = l} g[b][co] w[co][ci]     (0 elsewhere; every entry written)
 * x (b,cin,len), w (cout,cin), g (b,cout) = the gradient of v, idx (b,cout) int32 = the position
 * torch.max reported.  gx, gw may each be NULL (that gradient is not needed), gb too: each one that is given
 * is written, whichever others are (x is read for gw only, w for gx only).
 * len <= 16384, cout <= 4096, b <= 65535; gx needs (3 cout + len) * 4 <= 30000 (the sort of a cloud's winners
 * lives in LDS).  Fixed summation orders: bit-reproducible.  scratch (may be NULL):
 * mvp_pointwise_max_backward_scratch_bytes(...) bytes (0 = shape not covered by the staged pass: the same
 * LDS limit), contents irrelevant.  gw by one of two routes: with scratch of at least that size (and > 0) the
 * b * cout winning columns of x are staged there with coalesced accesses and then added; with scratch NULL,
 * too small, or a shape the staged pass does not cover, the columns are gathered directly (a 64-byte sector per
 * value).  Both add g[b][co] * column over the clouds in ascending order in one fmaf chain: the same bits.
 * gb is the plain sum of g over the clouds in ascending order, with or without gw.  The reference lets cuDNN
 * run its dense data- and weight-gradient passes on the max's gradient, a tensor of zeros. */
long long mvp_pointwise_max_backward_scratch_bytes(int b, int cin, int cout, int len);
int mvp_pointwise_max_backward(int b, int cin, int cout, int len, const float *x,
                               const float *w, const float *g, const int *idx,
                               float *gx, float *gw, float *gb, void *scratch,
                               long long scratch_bytes, void *stream);

/* ------------------------------------------------ registration (DCP) head */

/* Replaces the per-sample loop of SVDHead.forward
 * (registration/models/dcp.py:360-373, registration/model_utils.py:229-240):
 *   u, s, v = torch.svd(H[i]); r = v @ u.T; if det(r) < 0: r = (v @ diag(1,1,-1)) @ u.T
 * for all b matrices in one launch, no host synchronisation.
 * H (b,3,3) row-major -> R (b,3,3) the rotation (reflection fix applied);
 * optional (may be NULL): U (b,3,3), S (b,3) descending, V (b,3,3) with
 * H = U diag(S) V^T (V WITHOUT the fix), flipped (b) = 1 where the fix applied.
 * One-sided Jacobi in float64 per matrix, outputs rounded to float32.
 * Domain.  R is defined, and accurate to an ulp of 1.0, wherever the two smallest singular values do not
 * cancel behind the reflection (s_2 + d s_3 > 0, d = -1 where flipped): every H with det H > 0 down to rank 2,
 * coinciding singular values included (U and V are then one valid choice among many; R does not depend on
 * it), and every H with det H < 0 and s_3 < s_2.  At the poles of R (det H < 0 with s_2 = s_3, rank <= 1) the
 * result is a finite proper rotation, one of the equally good ones; the zero matrix gives the identity.
 * Every threshold is relative: scaling H by a power of two scales S and leaves R, U, V, flipped bit-equal.
 * float32 subnormals are read as they are, not as zeros.  A matrix holding a NaN or an Inf gets R = NaN in
 * all nine entries (never a plausible rotation) and the NaN / Inf in S; its U, V and flipped are unspecified;
 * no other matrix of the batch is affected.
 * The gradient of R with respect to H (registration.svd3_kabsch_backward, from U, S, V, flipped) is finite
 * on the same domain: it divides by s_a + s_b, and by s_a - s_3 where flipped, never by s_a^2 - s_b^2. */
int mvp_kabsch_svd3(int b, const float *H, float *R, float *U, float *S,
                    float *V, int *flipped, void *stream);

/* ------------------------------------- registration (DCP) transformer */

/* ABI 23.  The transformer's own normalisation (registration/models/dcp.py:139-149: `a_2 * (x - mean) / (std + eps) +
 * b_2`, std unbiased, eps added to the std -- not nn.LayerNorm) with the residual sum in front of it, one read and one
 * write of a row (two writes with the sum) where the reference runs two reductions, four elementwise passes and an
 * addition of its own.
 * x (rows,d); delta (rows,d) or NULL; a, b (d); sum (rows,d) or NULL, receives z = x + delta (one float add; z = x when
 * delta is NULL) and is required when delta is given; y (rows,d); stats (rows,2) or NULL, receives {mean, std} per row.
 * Per row:  mean = sum(z) / d (a true division),  c = z - mean,  std = sqrt(sum(c * c) / (d - 1)) from the CENTRED
 * values (never E[z^2] - mean^2),  y = (a * c) * (1 / (std + eps)) + b.
 * d % 4 == 0 and 4 <= d <= 1024, rows * d < 2^31 (else MVP_EBADSHAPE); eps >= 0 and finite, x / delta / sum / y 16-byte
 * aligned (else MVP_EBADARG); these refusals are decided before the null checks.  rows == 0 does nothing.
 * A constant row has std = 0 and y = b exactly (eps > 0).  A row that holds a NaN or an Inf gets y = NaN in all its d
 * entries (and NaN statistics); no other row changes.  One wave per row, fixed summation order: the same bits on every
 * run, on every device. */
int mvp_ref_layernorm(int rows, int d, const float *x, const float *delta, const float *a, const float *b, float eps,
                      float *sum, float *y, float *stats, void *stream);

/* Its backward pass, from z and the row statistics alone.  z (rows,d) = what was normalised (the forward's sum, or x);
 * gy (rows,d) the gradient of y; gres (rows,d) or NULL the gradient that reaches z directly, through the residual
 * stream; stats as written by the forward pass, eps the forward's.  With U = 1 / (std + eps), gh = gy * a:
 *   gz_i = U * (gh_i - mean(gh)) - c_i * (sum_j gh_j c_j) * U^2 / ((d - 1) * std)   [+ gres_i, the last single float add]
 *   ga[j] = sum_r gy[r,j] * c[r,j] * U_r,    gb[j] = sum_r gy[r,j]
 * The second term of gz is taken as 0 where std == 0 (what torch's std backward does: it masks a zero std).
 * c = z - mean is re-centred on the row's mean taken to double (stats' float32 mean is its first approximation), so a
 * centred value near the mean keeps its digits: ga over few rows depends on them.
 * gz, ga, gb are overwritten (rows == 0 writes nothing).  ga and gb may each be NULL; with both NULL no scratch is needed,
 * otherwise `scratch` holds mvp_ref_layernorm_backward_scratch_bytes(rows, d) bytes (16-byte aligned; one slab [2][d]
 * per workgroup, added in a fixed order by a second small launch: no atomics, bit-reproducible).  Shapes, alignment
 * (z, gy, gres, gz) and the order of the refusals as in the forward pass.  A non-finite row (NaN statistics) gets
 * gz = NaN in all its entries; a column of ga / gb is NaN if a contributing row is. */
long long mvp_ref_layernorm_backward_scratch_bytes(int rows, int d);
int mvp_ref_layernorm_backward(int rows, int d, const float *z, const float *a, const float *gy, const float *gres,
                               const float *stats, float eps, float *gz, float *ga, float *gb, void *scratch,
                               long long scratch_bytes, void *stream);

/* ------------------------------------ DGCNN's BatchNorm + ReLU + max over the neighbours, both ways (DCP training) */

/* BatchNorm2d (batch or running statistics) -> ReLU -> max over the neighbour axis of z (b,c,k,n), neighbours on the slow
 * axis and n contiguous (registration/models/dcp.py: DGCNN's stages; the reference composes conv, BatchNorm2d, ReLU and
 * max, dcp.py:286-318, and autograd keeps the BatchNorm's and the ReLU's outputs).  M = b k n values per channel:
 *   batch statistics:   mean_c = sum z / M,  var_c = sum (z - mean_c)^2 / M (biased, from CENTRED values),
 *                       invstd_c = 1 / sqrt(var_c + eps)
 *   running statistics: the caller fills stats with {running_mean_c, 1 / sqrt(running_var_c + eps)}
 *   y = fmaf(z - mean_c, gamma_c * invstd_c, beta_c),   r = relu(y),   pooled[b,c,n] = max_j r[b,c,j,n],
 *   arg[b,c,n] = the LOWEST j that attains it (uint8)
 * ReLU keeps a NaN; the maximum is NaN if a member is, and arg is then the lowest j that holds a NaN (torch's CPU rule).
 *
 * mvp_edge_bn_stats: z -> stats (c,2) = {mean, invstd} and var (c) = the biased variance (what the running variance is
 * updated from, times M / (M - 1)).  One workgroup per (b,c) slab of k n contiguous floats forms the slab's {mean, M2} in
 * double, M2 from values centred on the slab's own mean (the slab stays in registers up to 20480 floats, longer ones are
 * read twice); a second launch merges the b partials of a channel in ascending b with Chan's update, in double.  No
 * atomics: the same bits on every run.  `scratch` holds mvp_edge_bn_scratch_bytes(b, c) bytes, 16-byte aligned.
 *
 * mvp_edge_bn_relu_max: z, stats, gamma (c), beta (c) -> r (b,c,k,n) or nothing (r == NULL: nothing of z's size is
 * written), pooled (b,c,n), arg (b,c,n) uint8.  One workgroup per (b,c); a lane owns groups of four columns and walks k.
 *
 * Refusals, before anything is launched, in this order: MVP_EBADSHAPE for b < 1, c < 1, k outside 1..64, n < 4, n % 4 != 0,
 * k n >= 2^31 or b c >= 2^31; MVP_EBADARG for eps negative or not finite, for z, r, g_r, gz, pooled or g_pool off a
 * 16-byte address (arg: 4-byte), for a NULL required buffer and for scratch that is NULL, unaligned or too small.
 *
 * Non-finite values.  Batch statistics: a NaN or an Inf anywhere in a channel makes that channel's mean, invstd and var
 * NaN, hence all of its r, pooled and gz; no other channel changes by a bit.  Running statistics: the map is elementwise,
 * a NaN z[b,c,j,n] makes r[b,c,j,n] and pooled[b,c,n] NaN (an Inf gives y = +-Inf or, with gamma == 0, NaN) and nothing
 * else; its gz is 0 (the mask y > 0 is false for a NaN).
 * A dead channel (every y <= 0) gets r = 0, pooled = 0, arg = 0, gz = 0, ggamma = gbeta = 0, all exactly. */
long long mvp_edge_bn_scratch_bytes(int b, int c);
int mvp_edge_bn_stats(int b, int c, int k, int n, const float *z, float eps, float *stats, float *var, void *scratch,
                      long long scratch_bytes, void *stream);
int mvp_edge_bn_relu_max(int b, int c, int k, int n, const float *z, const float *stats, const float *gamma,
                         const float *beta, float *r, float *pooled, unsigned char *arg, void *stream);

/* Backward of the above from z, stats, gamma, beta and arg alone: r is no input, the ReLU mask is y > 0 with y recomputed by
 * the forward's own expression (bit-identical).  g_r (b,c,k,n) and g_pool (b,c,n) are the gradients of r and pooled; either
 * may be NULL (not both: MVP_EBADARG).
 *   g_y = (g_r + [j == arg] g_pool) where y > 0, else 0
 *   gbeta_c = sum g_y,   ggamma_c = sum g_y xhat,   xhat = (z - mean_c) invstd_c
 *   batch_stats != 0:  gz = gamma_c invstd_c (g_y - gbeta_c / M - xhat ggamma_c / M)
 *   batch_stats == 0:  gz = gamma_c invstd_c g_y
 * Pass 1 leaves per-slab sums of g_y and g_y xhat (double) in scratch, a small launch adds a channel's b partials in
 * ascending b and writes ggamma / gbeta (each may be NULL), pass 2 writes gz.  With running statistics and both sums
 * unwanted pass 1 is skipped (and no scratch is needed).  No atomics, bit-reproducible.  Refusals as above. */
int mvp_edge_bn_relu_max_backward(int b, int c, int k, int n, int batch_stats, const float *z, const float *stats,
                                  const float *gamma, const float *beta, const unsigned char *arg, const float *g_r,
                                  const float *g_pool, float *gz, float *ggamma, float *gbeta, void *scratch,
                                  long long scratch_bytes, void *stream);

/* ------------------------------------------- registration (DeepGMR) head */

/* Replaces get_rri_cluster's feature computation (registration/models/deepgmr.py:54-96):
 * rp, rq, theta in torch, then T_q and p/|p| copied to the host and the (B*M, S, k, k, 3)
 * np.cross / np.sum / np.arctan2 / np.argpartition temporaries there.
 * xyz (b,n,3), idx (b,n,k) int32 = the k neighbours of every point, self column already
 * dropped (knn(pts, k+1)[:, :, 1:]), each in [0, n) -> feat (b,4k,n): channel 4a+f holds
 * f in {rp = |p|, rq = |q_a|, theta = acos(clamp(p^.q^_a, -1, 1)), phi} of neighbour slot a,
 * the layout of the reference's cat(...).view(B,M,S,4k).transpose(1,3).  phi_a is the second
 * smallest of the multiset psi[a, 0..k-1] (psi[a,a] = 0 included), psi[a,b] =
 * remainder(atan2((T_b x T_a).p^, T_b.T_a), 2 pi) in float32, T_a = q_a - (p^.q^_a) p with the
 * unclamped dot.  2 <= k <= 64 (k < 2 -> MVP_EBADARG: the reference's argpartition fails).
 * Non-finite inputs: a point at the origin has no direction, so theta and phi of all its slots
 * are NaN; a neighbour at the origin makes theta and phi of that one slot NaN and takes no part
 * in the phi of the point's other slots (the clamp keeps a NaN, and phi is NaN where a row holds
 * fewer than two non-NaN psi), as the reference's clamp and NaN-last sort.  rp and rq stay
 * finite.  Never pi or inf in their place: a zero-padded cloud shows as NaN.
 * Forward only: the reference's phi goes through NumPy, no gradient reaches xyz. */
int mvp_rri_features(int b, int n, int k, const float *xyz, const int *idx, float *feat,
                     void *stream);

/* Replaces gmm_params (registration/models/deepgmr.py:98-121) and the softmax in front of it
 * (Model.forward :231-234: F.softmax(backbone(feats), dim=2)).
 * logits (b,j,n) = the backbone's last 1x1 convolution as it comes (no transposed copy) ->
 * gamma (b,n,j) = softmax over j (max-subtracted); pi (b,j) = mean_n gamma;
 * mu (b,j,3) = sum_n gamma p / (N pi); sigma (b,j) = the isotropic variance
 * sum_n gamma |p - mu|^2 / (N pi), two-pass (the reference's (b,j,3,3) is sigma * I).
 * 1 <= j <= 64 (else MVP_EBADARG), n >= 1.  Fixed summation orders, no atomics:
 * bit-reproducible. */
int mvp_gmm_params(int b, int n, int j, const float *logits, const float *xyz, float *gamma,
                   float *pi, float *mu, float *sigma, void *stream);

/* Backward of mvp_gmm_params with respect to the logits (no gradient to xyz):
 *   g_gamma[n][j] = g_pi_j / N + g_mu_j . (p_n - mu_j) / (N pi_j)
 *                   + g_sigma_j (|p_n - mu_j|^2 - sigma_j) / (N pi_j)
 * (sigma's dependence on mu drops out: sum_n gamma_nj (p_n - mu_j) = 0), then the softmax
 *   g_logits[j][n] = gamma_nj (g_gamma[n][j] - sum_j' gamma_nj' g_gamma[n][j']).
 * gamma, pi, mu, sigma: the forward's outputs; g_pi (b,j), g_mu (b,j,3), g_sigma (b,j) (all
 * required; pass zeros for an unused output) -> g_logits (b,j,n), every entry written. */
int mvp_gmm_params_backward(int b, int n, int j, const float *gamma, const float *xyz,
                            const float *pi, const float *mu, const float *sigma,
                            const float *g_pi, const float *g_mu, const float *g_sigma,
                            float *g_logits, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MVPOPS_H_ */
