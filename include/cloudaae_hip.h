/*
 * cloudaae_hip.h -- C ABI of libcloudaae_hip.so, the MI355X (gfx950) drop-in for
 * the native hot path of GeeeG/CloudAAE.
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer to contiguous row-major memory owned by
 *     the caller (outputs and workspaces included).  Two entry points take
 *     stream-ordered scratch of ONE call themselves (hipMallocAsync / hipFreeAsync
 *     on the caller's stream, nothing outlives the call): cloudaae_nn_distance*
 *     when it cuts a direction's candidates into ranges, and cloudaae_gemm_bf16x3
 *     for the planes of its second operand (cloudaae_gemm_bf16x3p takes them from
 *     the caller instead);
 *   - float = IEEE fp32, int = int32; sizes are element counts;
 *   - every function takes the HIP stream to launch on as its last argument
 *     (a hipStream_t passed as void*; NULL = the default stream), is re-entrant,
 *     never synchronises, and returns 0 or a hipError_t value
 *     (cloudaae_last_error() describes the most recent failure of the calling
 *     thread).  Process-wide state is limited to: the table of development knobs
 *     (cloudaae_set_knob; set them between launches, not concurrently with them),
 *     one low-priority side stream (cloudaae_side_stream), and per-device flags
 *     that record which kernels had their dynamic-LDS limit raised;
 *   - a workspace whose size comes from a cloudaae_*_workspace / *_partials query
 *     is only as large as the K split the knobs implied AT THE QUERY; the entry
 *     points that take one also take its size in floats and fail (no launch) when
 *     the cut they derive at launch time needs more -- e.g. after a change of
 *     CLOUDAAE_GEMM_SPLITS / CLOUDAAE_FC_FWD_SPLITS / CLOUDAAE_FC_FWD_BLOCKS /
 *     CLOUDAAE_DETERMINISTIC between the query and a launch or a replay;
 *   - gradient outputs are zero-filled by the callee.
 * The reference's launchers have C++ linkage, no stream and no status
 * (tf_nndistance.cpp:168,208; tf_sampling.cpp:65,94,125,150); each entry point
 * below names the one it replaces and keeps its argument order.
 */
#ifndef CLOUDAAE_HIP_H
#define CLOUDAAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *cloudaae_stream_t; /* hipStream_t */

/* The ABI revision this header describes: argument lists and struct layouts.  A caller built against another
 * revision must not call in -- check cloudaae_version() == CLOUDAAE_ABI_VERSION after loading (the Python host
 * does, cloudaae_amd/_lib.py).  500: round 5 (fully connected entry points take up to 128 rows; tickets / partials
 * queries take M; no y_zeroed argument).  600: round 6 (cloudaae_knn_hinted added; nothing else changed).
 * 601: cloudaae_selftest_div_by added.  602: cloudaae_icp_point_to_point and cloudaae_f64_to_f32 added; later, still
 * under 602 (additions only, no existing argument list or layout changed): cloudaae_frame_segments,
 * cloudaae_radius_outlier, cloudaae_ragged_fps and their workspace queries; cloudaae_dev_gemm_folded (development /
 * test entry); cloudaae_bn_backward_dx_bf16x3 and its two queries; cloudaae_pose_score, cloudaae_cloud_diameter (each with
 * a workspace query), cloudaae_pose_matrix and cloudaae_pose_stack; cloudaae_icp_point_to_plane and
 * cloudaae_estimate_normals with its workspace query; cloudaae_sample_poses and cloudaae_random_object_occluder;
 * cloudaae_vsd_counts and cloudaae_pose_max_dist with its workspace query; cloudaae_depth_normals and
 * cloudaae_depth_sensor_noise; cloudaae_frame_clouds with its workspace query and cloudaae_rendered_scene;
 * cloudaae_transform_hausdorff with its workspace query; cloudaae_nearest_equivalent_pose; cloudaae_pose_compose,
 * cloudaae_depth_fit_counts and cloudaae_select_pose; cloudaae_fc_plan (host-only path query); cloudaae_depth_plane,
 * cloudaae_depth_foreground, cloudaae_depth_components and cloudaae_component_labels, the last two with a workspace query;
 * cloudaae_depth_fit_counts_window and cloudaae_detect_assign; cloudaae_depth_creases with its workspace query;
 * cloudaae_depth_align_step with its workspace query; cloudaae_depth_edge_nearest, cloudaae_depth_contour_sums with its
 * workspace query and cloudaae_depth_align_solve; cloudaae_tsdf_integrate, cloudaae_tsdf_count and cloudaae_tsdf_emit;
 * cloudaae_tsdf_raycast; cloudaae_farthest_point_sample_variant, cloudaae_knn_variant and cloudaae_nn_distance_variant
 * (host-only queries: which kernel a call takes); cloudaae_tsdf_align_step with its workspace query. */
#define CLOUDAAE_ABI_VERSION 602
int cloudaae_version(void);
const char *cloudaae_last_error(void);
/* Development knobs (kernel A/B choices and launch shapes for tests and sweeps; none is needed in normal use):
 * an integer per name, initialised from the environment variable of the same name the first time the library
 * looks at it (the library never reads the environment again), changed with these two calls.  Names are listed
 * in DESIGN.md ("Development knobs"), e.g. "CLOUDAAE_KNN_SCAN", "CLOUDAAE_NN_FILTER".
 * One knob is a MODE rather than a tuning aid: "CLOUDAAE_DETERMINISTIC" = 1 keeps every product of cloudaae_gemm_* whole
 * over K (no slices added with atomics) and sorts the reverse neighbour lists of the edge convolution's backward pass;
 * together with cloudaae_nn_distance_grad_ordered and the GEMM + batch-norm route for the fully connected stack (the
 * host's choices: TrainGraph(deterministic=True)) a whole training step is then bit-reproducible from run to run, as
 * the reference's sequential CPU path is. */
int cloudaae_set_knob(const char *name, int value);
int cloudaae_unset_knob(const char *name);
/* Development helpers: what the instrumented library (`make prof`, a second shared object built with
 * -DCLOUDAAE_FC_PROFILE and -DCLOUDAAE_HPR_STATS) gathered, copied to HOST memory; the library as shipped carries no
 * instrumentation and both fail with hipErrorNotSupported.  They synchronise the device.
 * cloudaae_fc_profile_read: host[8192][8], the 100 MHz wall clock of the first 8192 workgroups at eight points of the
 *   fully connected kernels (tools/dev/fc_phases.py names the points); host NULL: no copy; clear != 0: zeroed afterwards.
 * cloudaae_hpr_stats_read: out[16], counters of cloudaae_hidden_point_removal (points, local re-solves, passes, box
 *   iterations, groups scanned, joined, fallbacks, vertices); reset != 0: zeroed afterwards. */
int cloudaae_fc_profile_read(unsigned long long *host, int clear);
int cloudaae_hpr_stats_read(unsigned long long *out, int reset);
/* HOST helper: CRC-32C (Castagnoli, reflected, init/final xor 0xffffffff) of n bytes of host memory -- the
 * checksum of the TFRecord framing (train_cloudAAE_ycbv.py:80-135) and of tf.train.Saver checkpoints
 * (:276, :418-430).  crc = 0 for a whole buffer, or the previous result to continue over the next piece. */
unsigned cloudaae_crc32c(const void *data, unsigned long long n, unsigned crc);

/* Two-stream plumbing.  cloudaae_side_stream(): a low-priority stream owned by the library (one per
 * process), for work off the critical path; NULL on failure.  cloudaae_stream_wait(waiter, signaller):
 * everything enqueued on `signaller` so far completes before anything enqueued on `waiter` from now on
 * (an event record + a stream wait; no host synchronisation).  A caller that hands a side stream to
 * cloudaae_edgeconv_backward, or launches on it itself, joins with cloudaae_stream_wait(main, side)
 * before it consumes the results. */
cloudaae_stream_t cloudaae_side_stream(void);
int cloudaae_stream_wait(cloudaae_stream_t waiter, cloudaae_stream_t signaller);

/* ---- tf_ops/nn_distance ------------------------------------------------- */

/* NnDistance forward, both directions in one launch.
 * Replaces: void NmDistanceKernelLauncher(int b,int n,const float* xyz,int m,
 *   const float* xyz2,float* result,int* result_i,float* result2,int* result2_i)
 *   (tf_ops/nn_distance/tf_nndistance.cpp:168, tf_nndistance_g.cu:128-131);
 * numerics of the CPU op (tf_nndistance.cpp:21-43): squared L2, un-fused fp32,
 * first minimum wins; m == 0 gives dist 0 / idx 0.
 * xyz1 [b,n,3], xyz2 [b,m,3] -> dist1 [b,n], idx1 [b,n], dist2 [b,m], idx2 [b,m].
 * Clouds of very unequal size take stream-ordered scratch (hipMallocAsync / hipFreeAsync on `stream`, nothing
 * outlives the call); the first such call raises the release threshold of the device's default memory pool so
 * that later calls reuse the memory instead of returning it to the driver at every synchronisation. */
int cloudaae_nn_distance(int b, int n, const float *xyz1, int m, const float *xyz2, float *dist1,
                         int *idx1, float *dist2, int *idx2, cloudaae_stream_t stream);
/* The same search when cloud c's xyz2 is `count2[c]` distinct points followed by copies of them -- the reference's own
 * Chamfer targets: the visible points, then random re-draws of visible points up to a fixed row count
 * (utils/hidden_point_removal.py:38-43, 72; sliced at train_cloudAAE_ycbv.py:211-214).  row_src2 [b,m] names, for every
 * row j >= count2[c], the row < count2[c] it is a bitwise copy of (cloudaae_hidden_point_removal_rows writes both).
 * Results are those of cloudaae_nn_distance bit for bit ("first index wins" puts every answer among the originals; a
 * copy's own answer is its original's), at the cost of the distinct points only.  count2[c] outside (0, m]: all m rows
 * are searched.  Both NULL: cloudaae_nn_distance.  A copy row whose row_src2 is not a distinct row (< 0, >= count2[c]) gets
 * dist2 = NaN and idx2 = 0 -- every output element is written; the development knob CLOUDAAE_NN_PREFIX_VERIFY = 1 also
 * compares every copy with its original bit for bit (NaN on a mismatch): the hint is only valid for targets that are still
 * what cloudaae_hidden_point_removal_rows wrote (no shuffle, slice beyond the rows, or augmentation in between). */
int cloudaae_nn_distance_prefix(int b, int n, const float *xyz1, int m, const float *xyz2, const long long *count2,
                                const int *row_src2, float *dist1, int *idx1, float *dist2, int *idx2,
                                cloudaae_stream_t stream);
/* Which search cloudaae_nn_distance / cloudaae_nn_distance_prefix run for these sizes, decided by the function the launch
 * itself calls (same thresholds, same knob CLOUDAAE_NN_FILTER, read at the time of the query): CLOUDAAE_NN_FILTER_KERNEL
 * (0) = the matrix-core filter with exact verification; 1, 2 or 4 = the plain search with that many queries per lane.
 * -1: sizes the entry points refuse, or for which they launch nothing.  Host only: launches nothing, touches no device
 * memory. */
#define CLOUDAAE_NN_FILTER_KERNEL 0
int cloudaae_nn_distance_variant(int b, int n, int m);

/* Development / test entry: the search scores of cloudaae_nn_distance's large-cloud kernel (|b'|^2 - 2 a'.b' of coordinates
 * centred on candidates[0], as error-free three-piece bfloat16 split products on the bf16 matrix pipe) for nq <= 32 queries
 * [nq,3] against nc <= 32 candidates [nc,3]: scores[q * 32 + c], and R[q] = (|a'_q| + max_c |b'_c|)^2, the quantity the
 * kernel's decision margin 160 * 2^-24 * R is stated in.  Same operand construction and instructions as the kernel. */
int cloudaae_dev_nn_split_scores(int nq, int nc, const float *queries, const float *candidates, float *scores, float *R,
                                 cloudaae_stream_t stream);

/* NnDistanceGrad.
 * Replaces: void NmDistanceGradKernelLauncher(int b,int n,const float* xyz1,int m,
 *   const float* xyz2,const float* grad_dist1,const int* idx1,const float* grad_dist2,
 *   const int* idx2,float* grad_xyz1,float* grad_xyz2)
 *   (tf_nndistance.cpp:208, tf_nndistance_g.cu:152-157; CPU loops tf_nndistance.cpp:126-163).
 * Either gradient output may be NULL (not wanted).  The terms of a point are added in no fixed order (atomics, in LDS per
 * 2048-point chunk of an output; the reference's own GPU kernel adds with global atomics): fp32 round-off apart from the
 * sequential sweep.  Every element of a wanted output is written. */
int cloudaae_nn_distance_grad(int b, int n, const float *xyz1, int m, const float *xyz2,
                              const float *grad_dist1, const int *idx1, const float *grad_dist2,
                              const int *idx2, float *grad_xyz1, float *grad_xyz2,
                              cloudaae_stream_t stream);
/* The same gradients accumulated in the ORDER of the reference's sequential CPU loops (tf_nndistance.cpp:126-163:
 * sweep over xyz1, then over xyz2), without atomics: bit-identical to that sweep and reproducible from run to run
 * (the atomic kernel above agrees with it to fp32 round-off only, as the reference's own GPU kernel does).
 * uniform != NULL: every distance has the upstream gradient uniform[0] * uniform_scale (the mean of
 * losses/chamfer_loss.py:13-14) and grad_dist1 / grad_dist2 are not read.  O(n m) index comparisons per cloud:
 * about ten times the time of the atomic kernel -- the deterministic mode's choice. */
int cloudaae_nn_distance_grad_ordered(int b, int n, const float *xyz1, int m, const float *xyz2,
                                      const float *grad_dist1, const int *idx1, const float *grad_dist2,
                                      const int *idx2, const float *uniform, float uniform_scale,
                                      float *grad_xyz1, float *grad_xyz2, cloudaae_stream_t stream);
/* The same when every distance has the SAME upstream gradient grad[0] * scale (the Chamfer loss is a mean
 * over them, losses/chamfer_loss.py:13-14): no per-point gradient arrays.  outputs_zeroed: only read by the
 * global-atomic development form (CLOUDAAE_NND_GRAD_LDS=0), which adds into its outputs (!= 0: the caller zero-filled
 * them, else the call clears them first); the default form stores every output element. */
int cloudaae_nn_distance_grad_uniform(int b, int n, const float *xyz1, int m, const float *xyz2, const float *grad,
                                      float scale, const int *idx1, const int *idx2, float *grad_xyz1,
                                      float *grad_xyz2, int outputs_zeroed, cloudaae_stream_t stream);

/* ---- tf_ops/sampling ---------------------------------------------------- */

/* FarthestPointSample: inp [b,n,3] -> out [b,m] (first index 0).
 * Replaces: void farthestpointsamplingLauncher(int b,int n,int m,const float* inp,
 *   float* temp,int* out) (tf_ops/sampling/tf_sampling.cpp:94, tf_sampling_g.cu:203-205;
 *   kernel :105-170, whose tie-break -- max, then lowest k mod 512, then lowest k --
 *   is reproduced).  `temp` is the reference's 32*n-float workspace
 *   (tf_sampling.cpp:115); it is only touched when n > 16384 and may be NULL
 *   otherwise. */
int cloudaae_farthest_point_sample(int b, int n, int m, const float *inp, float *temp, int *out,
                                   cloudaae_stream_t stream);
/* Which kernel cloudaae_farthest_point_sample runs for clouds of n points, decided by the function the launch itself
 * calls.  CLOUDAAE_FPS_BIG: the kernel for clouds above 16384 points (running minima in `temp`).  Otherwise
 * value & CLOUDAAE_FPS_PPT_MASK = the points a thread keeps in registers (1, 2, 4, 8, 16 or 32), and the bit
 * CLOUDAAE_FPS_XYZ_FROM_MEMORY is set when the cloud is too large for a copy in LDS, so that the coordinates of a
 * round's winner are read from memory.  -1: n <= 0.  Host only: launches nothing, touches no device memory. */
#define CLOUDAAE_FPS_PPT_MASK 0xff
#define CLOUDAAE_FPS_XYZ_FROM_MEMORY 0x100
#define CLOUDAAE_FPS_BIG 0x200
int cloudaae_farthest_point_sample_variant(int n);

/* GatherPoint: out[i,j,:] = inp[i,idx[i,j],:].
 * Replaces: void gatherpointLauncher(int b,int n,int m,const float* inp,const int* idx,
 *   float* out) (tf_sampling.cpp:125, tf_sampling_g.cu:172-181,206-208). */
int cloudaae_gather_point(int b, int n, int m, const float *inp, const int *idx, float *out,
                          cloudaae_stream_t stream);

/* GatherPointGrad: inp_g[i,idx[i,j],:] += out_g[i,j,:]; inp_g is zero-filled HERE
 * (the reference zeroes it in the Op, tf_sampling.cpp:174).
 * Replaces: void scatteraddpointLauncher(int b,int n,int m,const float* out_g,
 *   const int* idx,float* inp_g) (tf_sampling.cpp:150, tf_sampling_g.cu:183-192,209-211). */
int cloudaae_gather_point_grad(int b, int n, int m, const float *out_g, const int *idx,
                               float *inp_g, cloudaae_stream_t stream);

/* out[b,m] = for every draw inp_r[b,m] in [0,1) the smallest category whose inclusive prefix sum of
 * inp_p[b,n] reaches inp_r * total; temp[b*n] receives the prefix sums (the reference's workspace).
 * The prefix sums keep the reference's association order (quads, scan tree, compensated chunk
 * carry), so the indices are those of its kernels.  No gradient (tf_sampling.py:22).
 * Replaces: void probsampleLauncher(int b,int n,int m,const float* inp_p,const float* inp_r,
 *   float* temp,int* out) (tf_sampling.cpp:65, tf_sampling_g.cu:7-104,198-201). */
int cloudaae_prob_sample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp,
                         int *out, cloudaae_stream_t stream);

/* ---- utils/tf_util.py: kNN grouping ------------------------------------- */

/* pairwise_xyz_distance + knn fused (utils/tf_util.py:597-632): for every point
 * the k nearest points of its own cloud (self included), ascending distance,
 * ties -> lower index; the [b,n,n] matrix is never materialised.
 * x [b,n,ld] of which the first c channels are the metric (c = 3: the xyz slice
 * of tf_util.py:608; c = 64: the later layers); nn_idx [b,n,k].  k <= 32.
 * D[i][j] = (|x_i|^2 + (-2 * <x_i,x_j>)) + |x_j|^2 with <,> a channel-ordered
 * fp32 fma chain and |.|^2 a sequential un-fused sum (oracle_knn). */
int cloudaae_knn(int b, int n, int c, int ld, int k, const float *x, int *nn_idx,
                 cloudaae_stream_t stream);
/* Which kernel cloudaae_knn runs for these arguments, decided by the function the launch itself calls (same thresholds,
 * same knobs CLOUDAAE_KNN3_WIDE and CLOUDAAE_KNN_SCAN, read at the time of the query).  x_aligned: whether x sits on a
 * 16-byte boundary (the C = 64 kernels read rows as float4 and need it together with ld % 4 == 0).
 * value & 0xff = one of CLOUDAAE_KNN_* below; value >> 8 = the list length the kernel is built for (10, 20 or 32: the
 * smallest that holds k).  -1: arguments cloudaae_knn refuses, or for which it launches nothing.  Host only: launches
 * nothing, touches no device memory. */
#define CLOUDAAE_KNN_C3_WIDE 1    /* c = 3, matrix-core tiles, 16 waves per workgroup */
#define CLOUDAAE_KNN_C3_SCAN_1 2  /* c = 3, whole-cloud scan, one candidate range per query tile (four query tiles per workgroup) */
#define CLOUDAAE_KNN_C3_SCAN_2 3  /* ... two candidate ranges (two query tiles per workgroup) */
#define CLOUDAAE_KNN_C3_SCAN_4 4  /* ... four candidate ranges (one query tile per workgroup) */
#define CLOUDAAE_KNN_C64_WIDE 5   /* c = 64, bound pass + filtered scan, 16 waves per workgroup */
#define CLOUDAAE_KNN_C64_SCAN_1 6 /* c = 64, whole-cloud scan, one wave per query tile */
#define CLOUDAAE_KNN_C64_SCAN_2 7 /* c = 64, whole-cloud scan, two waves per query tile */
#define CLOUDAAE_KNN_GENERIC 8    /* any c, k and n: one lane per query */
int cloudaae_knn_variant(int b, int n, int c, int ld, int k, int x_aligned);
/* The same with a HINT (revision 600): hint [b,n,k] int32 = k DISTINCT indices per point that are likely to be near it -- the
 * neighbour lists of the layer before (models/pointnet_ycb_23_decoder_4.py:337-404 recomputes the lists layer by layer on
 * features that change little).  Their largest distance bounds the k-th distance, so the scan needs no bound pass of its
 * own.  The RESULT is cloudaae_knn's whatever the hint holds (a bad one costs time only).  tau_scratch: b * n floats.
 * Shapes outside the hinted kernel (c != 64, k > 20, clouds below 256 points, hint == NULL) take cloudaae_knn's path. */
int cloudaae_knn_hinted(int b, int n, int c, int ld, int k, const float *x, const int *hint, float *tau_scratch,
                        int *nn_idx, cloudaae_stream_t stream);

/* ---- utils/tf_util.py: dense layers ------------------------------------- */

/* C[M,N] (+)= op(A)[M,K] op(B)[K,N] (+ bias[N]); fp32 in / fp32 accumulate on the
 * matrix cores (v_mfma_f32_32x32x2_f32 = k-ordered fmaf chain).  Row-major.
 * trans_a: A is stored [K][M]; trans_b: B is stored [N][K].  accumulate: 0 overwrite C, 1 add to C,
 * 2 C already holds zeros (skips the clear pass of a split-K product).
 * Replaces tf.nn.conv2d 1x1 + bias_add (utils/tf_util.py:161-166) and tf.matmul +
 * bias_add (utils/tf_util.py:349-352) and their two gradient products. */
int cloudaae_gemm_f32(int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                      const float *B, int ldb, float *C, int ldc, const float *bias, int accumulate,
                      cloudaae_stream_t stream);
/* cloudaae_gemm_f32 (overwrite mode) that also leaves, per tile row of the product, the column sums and
 * sums of squares of C in fp64: colstats[parts][2][N], parts = cloudaae_gemm_f32_colstats_parts(M, N, K)
 * (0: this shape is split over K and has no such variant).  Feeds cloudaae_bn_forward_colstats. */
int cloudaae_gemm_f32_colstats_parts(int M, int N, int K);
int cloudaae_gemm_f32_colstats(int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                               const float *B, int ldb, float *C, int ldc, const float *bias, double *colstats,
                               cloudaae_stream_t stream);
/* K slices cloudaae_gemm_f32 will use for this shape (> 1: the output is combined with atomics and
 * must hold zeros first -- the call clears it itself unless accumulate is 1 or 2). */
int cloudaae_gemm_f32_splits(int M, int N, int K);
/* cloudaae_gemm_f32 (overwrite mode) whose result is BIT-REPRODUCIBLE from run to run: a product cut over K keeps
 * its slices apart in workspace (cloudaae_gemm_f32_ordered_workspace(M, N, K) floats; 0 = K stays whole and
 * workspace may be NULL) and a second kernel sums them in slice order, then adds the bias.  C need not be
 * cleared.  Used for every FORWARD product (the reference's CPU path is sequential and deterministic;
 * evaluate_cloudAAE_ycbv.py:421-477 returns the same reconstruction for the same frame). */
long long cloudaae_gemm_f32_ordered_workspace(int M, int N, int K);
int cloudaae_gemm_f32_ordered(int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                              const float *B, int ldb, float *C, int ldc, const float *bias, float *workspace,
                              long long workspace_floats, cloudaae_stream_t stream);
/* Several independent weight-gradient products C_j += A_j^T B_j (A_j stored [K][M], B_j [K][N]: dW = x^T dy of
 * utils/tf_util.py:161-166 for several layers) in ONE launch: each is a single wave of short split-K workgroups on its
 * own, and nothing waits for them before the optimiser.  C_j is added to with atomics and must hold zeros: zeroed != 0
 * says the caller cleared it, else the call does.  fold_c: 0, or the power-of-two width at which C's logical columns
 * fold into stacked row blocks (the edge convolution's [2*cin, cout] kernel used as [cin, 2*cout]); then ldc == fold_c. */
typedef struct cloudaae_gemm_tn_job {
    int M, N, K;
    const float *A;
    int lda;
    const float *B;
    int ldb;
    float *C;
    int ldc;
    int fold_c;
    int zeroed;
} cloudaae_gemm_tn_job;
int cloudaae_gemm_f32_tn_group(int count, const cloudaae_gemm_tn_job *jobs, cloudaae_stream_t stream);
/* cloudaae_gemm_f32_ordered with C's logical columns folded into stacked row blocks of width fold_c (as in
 * cloudaae_gemm_tn_job; 0: none), no bias: the edge convolution's weight gradients in deterministic mode. */
int cloudaae_gemm_f32_ordered_fold(int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                                   const float *B, int ldb, float *C, int ldc, int fold_c, float *workspace,
                                   long long workspace_floats,
                                   cloudaae_stream_t stream);
/* Development / test entry: cloudaae_gemm_f32 (bf16 == 0) or cloudaae_gemm_bf16 (bf16 != 0) without bias, with B and / or C
 * FOLDED as the edge convolution's products address its [2*cin, cout] kernel (used as [cin, 2*cout]): fold_b / fold_c = 0, or
 * the power-of-two width (>= 4) at which the logical columns fold into stacked row blocks -- logical (r, c) lives at row
 * (c / width) * rows + r, column c % width, rows = the logical row count (for B: of the matrix as stored, [K][N] or [N][K]);
 * the folded matrix has leading dimension == width.  Forwards to the launcher the edge convolution uses; no product code
 * calls it. */
int cloudaae_dev_gemm_folded(int bf16, int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                             const float *B, int ldb, float *C, int ldc, int accumulate, int fold_b, int fold_c,
                             cloudaae_stream_t stream);
/* The same product with both operands rounded to bfloat16 (round to nearest even) on their way
 * to the matrix cores (v_mfma_f32_32x32x16_bf16), fp32 accumulate; A, B, C, bias stay fp32 in
 * memory, so the call is interchangeable with cloudaae_gemm_f32 (BASELINE configs[2]: bf16 MLPs). */
int cloudaae_gemm_bf16(int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                       const float *B, int ldb, float *C, int ldc, const float *bias, int accumulate,
                       cloudaae_stream_t stream);
int cloudaae_gemm_bf16_splits(int M, int N, int K);
/* cloudaae_gemm_f32_ordered_workspace / _ordered for the bf16-operand product. */
long long cloudaae_gemm_bf16_ordered_workspace(int M, int N, int K);
int cloudaae_gemm_bf16_ordered(int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                               const float *B, int ldb, float *C, int ldc, const float *bias, float *workspace,
                               long long workspace_floats,
                               cloudaae_stream_t stream);
/* cloudaae_gemm_f32_colstats_parts / _colstats for the bf16-operand product. */
int cloudaae_gemm_bf16_colstats_parts(int M, int N, int K);
int cloudaae_gemm_bf16_colstats(int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                                const float *B, int ldb, float *C, int ldc, const float *bias, double *colstats,
                                cloudaae_stream_t stream);

/* fp32 products on the bf16 matrix cores by error-free splitting (opt-in; `gemm_dtype = "bf16x3"` in the Python host):
 * every operand element is split exactly into three bfloat16 pieces and the six piece products of weight >= 2^-16
 * are accumulated in fp32 -- what is dropped is below 2^-23 of each product, the size of one fp32 rounding, so the
 * result agrees with cloudaae_gemm_f32 at the level of an fp32 accumulation in another order -- at 2.7 x less matrix-pipe
 * time (six 32-cycle bf16 MFMAs per 16 k against eight 64-cycle fp32 MFMAs).  Arguments as cloudaae_gemm_f32 plus the
 * optional column sums of cloudaae_gemm_f32_colstats (cloudaae_gemm_bf16x3_colstats_parts tile rows).  Served: whole
 * tiles of 128 / 160, K % 32 == 0, 16-byte aligned rows, not both operands transposed
 * (cloudaae_gemm_bf16x3_supported); accumulate: 0 overwrite, 1 add, 2 add into a C the caller cleared. */
int cloudaae_gemm_bf16x3_supported(int trans_a, int trans_b, int M, int N, int K);
int cloudaae_gemm_bf16x3_colstats_parts(int M, int N, int K);
int cloudaae_gemm_bf16x3(int trans_a, int trans_b, int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                         float *C, int ldc, const float *bias, int accumulate, double *colstats, cloudaae_stream_t stream);
/* The same split products with the second operand split ONCE by the caller (a weight multiplies every row tile of a
 * step's forward AND backward product): cloudaae_x3_split writes the three bfloat16 planes of a [rows][k] matrix
 * (src = [rows][k], or [k][rows] when transposed != 0; cloudaae_x3_planes_bytes(rows, k) = 6 rows k bytes, 16-byte
 * aligned, k % 32 == 0) in the order the matrix cores read them, and cloudaae_gemm_bf16x3p computes
 * C[M,N] (+)= A[M,K] P^T (+ bias) with P the planes of the [N][K] operand -- y = x W with the planes of W^T
 * (cloudaae_x3_split(N, K, W, ldw, 1, ..)), dx = dy W^T with the planes of W (cloudaae_x3_split(K_w, N_w, W, ldw, 0, ..)).
 * A stays fp32 and is split in registers, once per element.  Served: M % 128 == 0, N a multiple of 128 or 160,
 * K % 32 == 0, rows of A 16-byte aligned (cloudaae_gemm_bf16x3p_supported); colstats as cloudaae_gemm_f32_colstats with
 * cloudaae_gemm_bf16x3p_colstats_parts(M, N, K) tile rows.  cloudaae_gemm_bf16x3 itself takes this route for
 * trans_a == 0 with planes in stream-ordered scratch of the call. */
long long cloudaae_x3_planes_bytes(int rows, int k);
int cloudaae_x3_split(int rows, int k, const float *src, int ld, int transposed, void *planes, cloudaae_stream_t stream);
/* both plane sets of a weight W[K][N] in one launch: planes_fwd = cloudaae_x3_split(N, K, W, ldw, 1, ..) for y = x W,
 * planes_bwd = cloudaae_x3_split(K, N, W, ldw, 0, ..) for dx = dy W^T (6 K N bytes each; K, N multiples of 32) */
int cloudaae_x3_split_weight(int K, int N, const float *W, int ldw, void *planes_fwd, void *planes_bwd,
                             cloudaae_stream_t stream);
int cloudaae_gemm_bf16x3p_supported(int M, int N, int K);
int cloudaae_gemm_bf16x3p_colstats_parts(int M, int N, int K);
int cloudaae_gemm_bf16x3p(int M, int N, int K, const float *A, int lda, const void *planes, float *C, int ldc,
                          const float *bias, int accumulate, double *colstats, cloudaae_stream_t stream);

/* Batch-norm backward of a mean-pooled layer (cloudaae_bn_backward with pool_mode 1 and no dout) AND the input-gradient
 * product of the linear layer in front of it, dx[M,N] = dy[M,C] P^T (cloudaae_gemm_bf16x3p with the planes of the [N][C]
 * weight), as one call: the per-channel sums are finalised as ever, but the pass that would read y and write dy is gone --
 * the product reads y, forms every dy element in registers (the same fp32 operations in the same order) on its way into the
 * matrix cores, and its first column tile stores dy for the weight-gradient product.  dy, dx, dgamma, dbeta, dbias are
 * bit-identical to the two calls.  Served (cloudaae_bn_backward_dx_bf16x3_supported): C % 32 == 0, N % 160 == 0 and
 * N % 128 != 0, M % 128 == 0, pool_rows % 128 == 0 (a 128-row tile inside one pooling group); anything else is refused.
 * consts: scratch of cloudaae_bn_backward_dx_bf16x3_consts_bytes(M, C, pool_rows) bytes, 16-byte aligned. */
int cloudaae_bn_backward_dx_bf16x3_supported(int M, int C, int N, int pool_rows);
long long cloudaae_bn_backward_dx_bf16x3_consts_bytes(int M, int C, int pool_rows);
int cloudaae_bn_backward_dx_bf16x3(int M, int C, const float *y, int ldy, const float *gamma, const float *beta,
                                   const float *save_mean, const float *save_var, int training, int relu, int pool_rows,
                                   const float *dpooled, float *dy, int lddy, float *dgamma, float *dbeta, float *dbias,
                                   int accumulate_param_grads, const double *pool_stats, void *workspace, void *consts,
                                   int N, const void *planes, float *dx, int lddx, cloudaae_stream_t stream);

/* ---- activations kept as bfloat16 in HBM (BASELINE configs[2]: "bf16 MLPs") --------------------------------------
 * The same products as cloudaae_gemm_bf16 (conv2d 1x1 and its two gradient products, utils/tf_util.py:161-166) with
 * operands that already ARE bfloat16 in memory (uint16_t = the upper half of the fp32 pattern, round to nearest
 * even), fp32 accumulate; C is fp32, or bfloat16 when c_is_bf16 != 0.  Served: whole tiles only --
 * cloudaae_gemm_b16_supported() says whether (trans_a, trans_b, M, N, K) is (K % 64 == 0, M and N multiples of the
 * 128 / 160 tile sides, not both operands transposed); rows of A, B (and of a bf16 C) 16-byte aligned.
 * colstats (optional, as cloudaae_gemm_f32_colstats, cloudaae_gemm_b16_colstats_parts(M, N, K) tile rows): column
 * sums and sums of squares of the fp32 values C was rounded from.  accumulate: 0 overwrite, 1 add to C (fp32 C). */
int cloudaae_gemm_b16_supported(int trans_a, int trans_b, int M, int N, int K);
int cloudaae_gemm_b16_colstats_parts(int M, int N, int K);
int cloudaae_gemm_b16(int trans_a, int trans_b, int M, int N, int K, const uint16_t *A, int lda, const uint16_t *B,
                      int ldb, void *C, int ldc, int c_is_bf16, const float *bias, int accumulate, double *colstats,
                      cloudaae_stream_t stream);
/* dst[i] = bfloat16(src[i]) (round to nearest even), n a multiple of 8, both 16-byte aligned. */
int cloudaae_to_bf16(long long n, const float *src, uint16_t *dst, cloudaae_stream_t stream);
/* batch_norm_template + ReLU + reduce_mean over groups of pool_rows rows (models/pointnet_ycb_23_decoder_4.py:
 * 410-419) in training mode on a bfloat16 y[M,C]: the moments come from `colstats` (the fp32 column sums the product
 * left), the EMA shadows are updated, pooled[M/pool_rows, C] and pool_stats[M/pool_rows][3][C] are written as by
 * cloudaae_bn_forward_colstats(pool_mode 1, relu).  C % 256 == 0, pool_rows % 64 == 0. */
int cloudaae_bn_meanpool_forward16(int M, int C, const uint16_t *y, int ldy, const float *gamma, const float *beta,
                                   const float *decay, float *ema_mean, float *ema_var, float *save_mean,
                                   float *save_var, int pool_rows, float *pooled, double *pool_stats, void *workspace,
                                   const double *colstats, int colstats_parts, cloudaae_stream_t stream);
/* Its gradient: dy[M,C] (bfloat16) from dpooled[M/pool_rows, C]; dgamma / dbeta / dbias as cloudaae_bn_backward. */
int cloudaae_bn_meanpool_backward16(int M, int C, const uint16_t *y, int ldy, const float *gamma, const float *beta,
                                    const float *save_mean, const float *save_var, int pool_rows, const float *dpooled,
                                    uint16_t *dy, int lddy, float *dgamma, float *dbeta, float *dbias,
                                    int accumulate_param_grads, const double *pool_stats, void *workspace,
                                    cloudaae_stream_t stream);

/* batch_norm_template (utils/tf_util.py:473-511) on rows y[M,C] (+ ReLU), writing the
 * activation out[M,C] and/or its pool over groups of pool_rows consecutive rows
 * (pool_mode 0 none, 1 mean = models/pointnet_ycb_23_decoder_4.py:419, 2 max = :684,
 * :59-60; tie_count[M/pool_rows,C] receives the number of equal maxima).
 * training != 0: batch moments (biased variance), EMA shadows updated as
 * s -= (s - stat) * (1 - decay[0]) when ema_mean != NULL; training == 0: moments =
 * EMA shadows.  save_mean/save_var[C] receive the moments used.  eps = 1e-3.
 * workspace: cloudaae_bn_workspace_bytes(C) bytes.  * pool_stats (optional, mean pool + ReLU in training mode): 3 x C doubles per group -- rows passing the
 * ReLU, sum of their x_hat, sum of all x_hat -- which cloudaae_bn_backward(pool_stats=...) turns into its
 * column sums without a pass over y when the pooled value is the only consumer (dout == NULL). */
long long cloudaae_bn_workspace_bytes(int C);
int cloudaae_bn_forward(int M, int C, const float *y, int ldy, const float *gamma, const float *beta,
                        int training, const float *decay, float *ema_mean, float *ema_var,
                        float *save_mean, float *save_var, int relu, float *out, int ldo, int pool_rows,
                        int pool_mode, float *pooled, float *tie_count, double *pool_stats, void *workspace,
                        cloudaae_stream_t stream);
/* The same with the statistics pass skipped: colstats[colstats_parts][2][C] already holds per-row-tile
 * column sums / sums of squares of y, written by cloudaae_gemm_f32_colstats (the product that made y had
 * the tile in registers anyway: for dgcnn_agg this saves reading 134 MB). */
int cloudaae_bn_forward_colstats(int M, int C, const float *y, int ldy, const float *gamma, const float *beta,
                                 int training, const float *decay, float *ema_mean, float *ema_var,
                                 float *save_mean, float *save_var, int relu, float *out, int ldo, int pool_rows,
                                 int pool_mode, float *pooled, float *tie_count, double *pool_stats, void *workspace,
                                 const double *colstats, int colstats_parts, cloudaae_stream_t stream);
/* gradient of the above: upstream = dout[M,C] (may be NULL) and/or dpooled[M/pool_rows,C]
 * (mean: /pool_rows; max: shared among equal maxima, as tf.reduce_max does);
 * produces dy[M,C], dgamma[C], dbeta[C] (NULL = not wanted), and dbias[C] (NULL = not wanted): the
 * gradient of a bias added to y right before the batch norm (tf_util.py:166 / :352 followed by
 * :173 / :355), i.e. the column sums of dy, without another pass over dy. */
int cloudaae_bn_backward(int M, int C, const float *y, int ldy, const float *gamma, const float *beta,
                         const float *save_mean, const float *save_var, int training, int relu,
                         const float *dout, int lddo, int pool_rows, int pool_mode, const float *dpooled,
                         const float *pooled, const float *tie_count, float *dy, int lddy, float *dgamma,
                         float *dbeta, float *dbias, int accumulate_param_grads, const double *pool_stats,
                         void *workspace, cloudaae_stream_t stream);
/* ---- batch norm over a batch that is sharded across ranks (SyncBN) -------------------
 * The reference is single-GPU: tf.nn.moments (utils/tf_util.py:492) sees the WHOLE batch.  When the
 * batch is sharded data-parallel, the `_sync` variants below reproduce that: every rank reduces its rows
 * to per-channel fp64 sums, the HOST-SUPPLIED `allreduce` adds them across ranks (the library does not
 * link a communication library; the host passes RCCL, or anything else, through its own runtime), and
 * the moments / the backward means are taken over count x world rows.  dgamma, dbeta and the bias gradient
 * stay LOCAL sums (the gradient exchange adds them across ranks like every other parameter gradient);
 * the EMA shadows see the global moments, so they stay identical on every rank.
 *   allreduce(ctx, buf, count, stream): sum `count` doubles at device pointer `buf` over all ranks, in
 *     place, ordered after the work already enqueued on `stream` and before whatever is enqueued next;
 *     returns 0 on success.  Called once per forward and once per backward of a layer.
 *   buf: device scratch of at least 2*C doubles owned by the caller (the sums travel in it).
 *   world: number of ranks (every rank contributes the same number of rows).
 * sync == NULL: exactly the plain entry point. */
typedef int (*cloudaae_allreduce_fn)(void *ctx, double *buf, int count, cloudaae_stream_t stream);
typedef struct cloudaae_bn_sync {
    cloudaae_allreduce_fn allreduce;
    void *ctx;
    int world;
    double *buf;
} cloudaae_bn_sync;
/* cloudaae_bn_forward / _colstats (colstats may be NULL) with global moments */
int cloudaae_bn_forward_sync(int M, int C, const float *y, int ldy, const float *gamma, const float *beta,
                             int training, const float *decay, float *ema_mean, float *ema_var,
                             float *save_mean, float *save_var, int relu, float *out, int ldo, int pool_rows,
                             int pool_mode, float *pooled, float *tie_count, double *pool_stats, void *workspace,
                             const double *colstats, int colstats_parts, const cloudaae_bn_sync *sync,
                             cloudaae_stream_t stream);
/* cloudaae_bn_backward with the means of (dz, dz*x_hat) over the global batch */
int cloudaae_bn_backward_sync(int M, int C, const float *y, int ldy, const float *gamma, const float *beta,
                              const float *save_mean, const float *save_var, int training, int relu,
                              const float *dout, int lddo, int pool_rows, int pool_mode, const float *dpooled,
                              const float *pooled, const float *tie_count, float *dy, int lddy, float *dgamma,
                              float *dbeta, float *dbias, int accumulate_param_grads, const double *pool_stats,
                              void *workspace, const cloudaae_bn_sync *sync, cloudaae_stream_t stream);
/* cloudaae_edgeconv_forward / _backward (declared below) with the batch norm of the block over the edges of
 * every rank's clouds: same arguments plus `sync` in front of the stream(s). */
int cloudaae_edgeconv_forward_sync(int b, int n, int k, int cin, int cout, const float *x, int ldx,
                                   const int *nn_idx, const float *weights, const float *biases,
                                   const float *gamma, const float *beta, int training, const float *decay,
                                   float *ema_mean, float *ema_var, int pool_mode, float *pq, float *save_mean,
                                   float *save_var, float *out, int ldo, float *tie_count, float *edge_stats,
                                   int gemm_bf16, void *workspace, const cloudaae_bn_sync *sync,
                                   cloudaae_stream_t stream);
int cloudaae_edgeconv_backward_sync(int b, int n, int k, int cin, int cout, const float *x, int ldx,
                                    const int *nn_idx, const float *weights, const float *biases,
                                    const float *gamma, const float *beta, int training, int pool_mode,
                                    const float *pq, const float *save_mean, const float *save_var,
                                    const float *out, int ldo, const float *tie_count, const float *dout, int lddo,
                                    float *dpq, int *rev_scratch, int rev_ready, float *dx, int lddx,
                                    int accumulate_dx, float *dweights, int dweights_zeroed, float *dbiases,
                                    float *dgamma, float *dbeta, const float *edge_stats, int gemm_bf16,
                                    void *workspace, const cloudaae_bn_sync *sync, cloudaae_stream_t stream,
                                    cloudaae_stream_t side_stream);
/* out[c] (+)= sum_r x[r][c] (bias gradients); workspace as for bn (same C). */
int cloudaae_colsum_f32(int M, int C, const float *x, int ldx, float *out, int accumulate, void *workspace,
                        cloudaae_stream_t stream);

/* ---- a whole fully connected layer at small batch ------------------------ */

/* tf_util.fully_connected (utils/tf_util.py:321-365: tf.matmul :351, bias_add :352, batch_norm_for_fc
 * :355, activation :358) as ONE launch per direction when the rows are the clouds of a batch of at
 * most cloudaae_fc_max_rows() (= 128: four 32-row MFMA tiles): the decoder and pose heads of
 * models/pointnet_ycb_23_decoder_4.py:413-455.  Larger batches take cloudaae_gemm_f32 + cloudaae_bn_*.
 *
 * forward: y[M,N] = x[M,K] w[K,N] + bias (bias may be NULL); with gamma != NULL also the batch norm of
 * y (arguments as cloudaae_bn_forward) into out[M,N], y keeping the pre-normalisation values the
 * backward needs.  gamma == NULL: no batch norm, only y is written, and `relu` is ignored in both directions
 * (there is no activation without the batch norm: dout is then the gradient of y as it is).
 * tickets: cloudaae_fc_forward_tickets(M, N) ints holding ZERO, left zero by the call (arrival counters:
 * the product is cut over K -- and over 32-row tiles of the batch -- across workgroups; the last to
 * arrive at a column tile sums the pieces and, with batch norm, normalises the column tile);
 * partials: cloudaae_fc_forward_partials(M, K, N, gamma != NULL) floats of scratch (any contents);
 * partials_floats: the floats behind it (the call fails if this launch's cut needs more -- the cut is derived again
 * at every launch, also from development knobs).
 * The pieces are summed in a FIXED order by the last to arrive: the layer is bit-reproducible from run
 * to run.  With tickets or partials NULL a layer keeps K whole in one workgroup per column tile and
 * row tile (slower; batch norm over more than 32 rows is then refused).
 * Two calls in flight at the same time (different streams) need separate counters and scratch. */
int cloudaae_fc_max_rows(void);
int cloudaae_fc_forward_tickets(int M, int N);
long long cloudaae_fc_forward_partials(int M, int K, int N, int batch_norm);
/* Which kernel path a layer of these sizes takes (host only, launches nothing; what the launch code derives, from the
 * same helpers).  batch_norm: gamma != NULL; vec: the launch would find its pointers 16-byte aligned and its sizes whole
 * quads (forward: K % 8 == 0, ldx % 4 == 0, N % 4 == 0, x and w aligned; backward: N % 4 == 0, w and dw aligned);
 * scratch: tickets and partials are given.  Six ints into out:
 *   forward : cq (columns per lane: tiles of 32 cq columns), tiles (column tiles), rts (32-row tiles), splits (K slices),
 *             kslice (k per slice), combine (partial tiles meet in the scratch)
 *   backward: RT (row tiles the kernel is built for: 1, 2 or 4), fine (four waves share a tile of W) or not (a wave per
 *             tile), parts (4 or 2 accordingly), tiles_per_block, by (workgroups per 128-column slice), staged (W read
 *             in whole lines through LDS: vec, one row tile, not fine)
 * Returns 0, or 1 for sizes the entry points refuse. */
int cloudaae_fc_plan(int backward, int M, int K, int N, int batch_norm, int vec, int scratch, int *out);
int cloudaae_fc_forward(int M, int K, int N, const float *x, int ldx, const float *w, const float *bias,
                        const float *gamma, const float *beta, int training, const float *decay,
                        float *ema_mean, float *ema_var, float *save_mean, float *save_var, int relu,
                        float *y, float *out, int *tickets, float *partials,
                        long long partials_floats, cloudaae_stream_t stream);
/* backward of the same layer from dout[M,N] (gradient of `out`, or of y when gamma == NULL):
 *   dx[M,K] += d(y) w^T      (ADDED with fp32 atomics: pass zeros, or a buffer that other consumers
 *                             of x add their gradients to as well; NULL = not wanted)
 *   dw[K,N] (+)= x^T d(y)    (accumulate_dw; NULL = not wanted)
 *   dgamma, dbeta, dbias (+)= as cloudaae_bn_backward (accumulate_param_grads; NULL = not wanted;
 *                             without batch norm dbias = column sums of dout). */
int cloudaae_fc_backward(int M, int K, int N, const float *x, int ldx, const float *w, const float *y,
                         const float *gamma, const float *beta, const float *save_mean,
                         const float *save_var, int training, int relu, const float *dout, int lddo,
                         float *dx, int lddx, float *dw, int accumulate_dw, float *dgamma, float *dbeta,
                         float *dbias, int accumulate_param_grads, cloudaae_stream_t stream);

/* Up to cloudaae_fc_max_group() (= 4) INDEPENDENT layers of the same batch in one launch per
 * direction: the decoder and the two pose heads are three chains of three layers
 * (models/pointnet_ycb_23_decoder_4.py:413-455), so depth by depth they are three launches forward and
 * three backward instead of nine each.  One record per layer, fields as the arguments of
 * cloudaae_fc_forward / cloudaae_fc_backward above (forward reads the first block, backward both).
 * Layers that share their input x may share dx: the gradients of all consumers add up in it. */
typedef struct cloudaae_fc_layer {
    int K, N;
    const float *x;
    int ldx;
    const float *w, *bias;
    const float *gamma, *beta;          /* gamma NULL: no batch norm */
    float *ema_mean, *ema_var, *save_mean, *save_var;
    int relu;
    float *y, *out;
    int *tickets;
    /* backward */
    const float *dout;
    int lddo;
    float *dx;
    int lddx;
    float *dw;
    int accumulate_dw;
    float *dgamma, *dbeta, *dbias;
    int accumulate_param_grads;
    /* forward */
    float *partials;
    long long partials_floats;          /* floats behind `partials` (>= cloudaae_fc_forward_partials at launch time) */
    const float *out_rowvec;            /* gamma NULL only: y[r][c] += out_rowvec[r * out_rowvec_d + c % out_rowvec_d] */
    int out_rowvec_d;                   /* (train_cloudAAE_ycbv.py:232-233: xyz_recon = recon_res + element_mean) */
} cloudaae_fc_layer;
int cloudaae_fc_max_group(void);
int cloudaae_fc_forward_group(int M, int count, const cloudaae_fc_layer *layers, int training,
                              const float *decay, cloudaae_stream_t stream);
int cloudaae_fc_backward_group(int M, int count, const cloudaae_fc_layer *layers, int training,
                               cloudaae_stream_t stream);

/* ---- the DGCNN edge-convolution block, fused ---------------------------- */

/* get_edge_feature + conv2d 1x1 + batch norm + ReLU + pool over k
 * (utils/tf_util.py:635-669,111-179; models/pointnet_ycb_23_decoder_4.py:337-350):
 * x[b*n, cin] (row stride ldx), nn_idx[b,n,k], weights[2*cin, cout] (the TF kernel
 * [1,1,2cin,cout]), pool_mode 1 mean / 2 max -> out[b*n, cout] (row stride ldo).
 * pq[b*n, 2*cout] is scratch that the backward pass reads again.  cout in {64,128}.
 * max pool: tie_count[b*n, cout] receives the number of equal maxima (tf.reduce_max shares
 * the gradient among them); backward then also needs the forward output.
 * backward scratch: dpq[b*n, 2*cout] floats, rev_scratch[b*(n+1) + b*n*k] ints (reverse
 * neighbour lists, built by a counting sort in LDS: no atomics on the gradient tensors).
 * gemm_bf16 != 0: the block's dense products round their operands to bfloat16 (cloudaae_gemm_bf16).
 * dweights_zeroed != 0: the caller already cleared dweights (skips the clear pass of the split-K products).  * edge_stats (optional, used with mean pool in training mode): [b*n][3][cout] floats the forward call
 * fills per point -- edges passing the ReLU, sum of their x_hat, sum of all x_hat -- and the backward
 * call, given the same buffer, turns into its column sums with a streaming pass instead of gathering
 * every neighbour again (24.7 -> 7 us per 64-channel layer at B=32, N=1024).  * pq: [b*n][2*cout] scratch of the call; on return its first cout columns hold U = X W_centre' + b
 * (centre term of every edge of the point) and the last cout columns Q = X W_neighbour, which is how
 * cloudaae_edgeconv_backward expects to find it. */
long long cloudaae_edgeconv_workspace_bytes(int cout);
/* Self-test of the gradient pass's division by the neighbour count (mean pooling, utils/tf_util.py reduce_mean over k:
 * models/pointnet_ycb_23_decoder_4.py:350): the kernels divide by a launch-wide constant d with the IEEE sequence's
 * d-only part (reciprocal and its refinement, scaling of d) computed once -- six or eight instructions per quotient
 * instead of eleven.  Walks ALL 2^32 float numerators x: count[0] = those whose quotient differs in its bits from x / d
 * (two NaNs are equal), count[1] = bits of the largest magnitude among them.  count: 2 x u64, device memory.
 * corrections: 1 or 2 remainder steps; 0 = what cloudaae_edgeconv_backward takes for k = d.  1 <= d <= 2^20. */
int cloudaae_selftest_div_by(float d, int corrections, unsigned long long *count, cloudaae_stream_t stream);
int cloudaae_edgeconv_forward(int b, int n, int k, int cin, int cout, const float *x, int ldx,
                              const int *nn_idx, const float *weights, const float *biases,
                              const float *gamma, const float *beta, int training, const float *decay,
                              float *ema_mean, float *ema_var, int pool_mode, float *pq, float *save_mean,
                              float *save_var, float *out, int ldo, float *tie_count, float *edge_stats,
                              int gemm_bf16, void *workspace, cloudaae_stream_t stream);
/* The same, the pooled output stored once more as bfloat16 (round to nearest even, the conversion of cloudaae_to_bf16):
 * out_bf16 [b*n] rows ldo_bf16 elements apart -- a column slice of the bfloat16 twin of the concat buffer the aggregation
 * product reads when activations are kept in bfloat16 (BASELINE configs[2]): no conversion pass over the concat. */
int cloudaae_edgeconv_forward_b16out(int b, int n, int k, int cin, int cout, const float *x, int ldx,
                                     const int *nn_idx, const float *weights, const float *biases,
                                     const float *gamma, const float *beta, int training, const float *decay,
                                     float *ema_mean, float *ema_var, int pool_mode, float *pq, float *save_mean,
                                     float *save_var, float *out, int ldo, float *tie_count, float *edge_stats,
                                     int gemm_bf16, void *workspace, void *out_bf16, int ldo_bf16,
                                     cloudaae_stream_t stream);
/* Reverse neighbour lists (for every point m: the points that have m among their k neighbours) of up to 8
 * layers in one launch: rev_scratch[i] (b*(n+1) + b*n*k ints, the buffer later passed to
 * cloudaae_edgeconv_backward with rev_ready = 1) from nn_idx[i] ([b,n,k]).  The encoder's layers all have
 * their neighbour lists by the end of the forward pass, so backward builds them together. */
int cloudaae_edgeconv_revlists(int count, int b, int n, int k, const int *const *nn_idx, int *const *rev_scratch,
                               cloudaae_stream_t stream);
int cloudaae_edgeconv_backward(int b, int n, int k, int cin, int cout, const float *x, int ldx,
                               const int *nn_idx, const float *weights, const float *biases,
                               const float *gamma, const float *beta, int training, int pool_mode,
                               const float *pq, const float *save_mean, const float *save_var,
                               const float *out, int ldo, const float *tie_count, const float *dout,
                               int lddo, float *dpq, int *rev_scratch, int rev_ready, float *dx, int lddx,
                               int accumulate_dx, float *dweights, int dweights_zeroed, float *dbiases,
                               float *dgamma, float *dbeta, const float *edge_stats, int gemm_bf16,
                               void *workspace, cloudaae_stream_t stream, cloudaae_stream_t side_stream);

/* ---- train_cloudAAE_ycbv.py:194-273: the step around the network --------- */

/* :206-226  pc[b,n,3+num_class] = [visible[:, :n] + noise - mean, one_hot(class_id)],
 * mean[b,3] over the n noisy points; noisy[b,n,3] optional; visible is [b,p,3], p >= n. */
int cloudaae_input_assemble(int b, int p, int n, int num_class, const float *visible, const float *noise,
                            const long long *class_id, float *pc, float *mean, float *noisy,
                            cloudaae_stream_t stream);
/* The same with the noise of :217 (tf.random.normal, stddev = noise_std) drawn INSIDE the kernel: Philox4x32-10 keyed by
 * `seed`, counter = (cloud, point), stream = draws[0] -- the number of launches that have drawn so far, kept in the two
 * 64-bit device words `draws` ({counter, arrival ticket}, both zero to start with; the last workgroup of a launch
 * advances the counter, so a recorded step replayed with the same arguments draws fresh noise every time and the noise
 * does not depend on the global-step variable).  Same distribution as the reference's generator, not the same stream.
 * draws == NULL: stream 0 at every launch. */
int cloudaae_input_assemble_noise(int b, int p, int n, int num_class, const float *visible, const long long *class_id,
                                  float *pc, float *mean, float *noisy, float noise_std, unsigned long long seed,
                                  unsigned long long *draws, cloudaae_stream_t stream);
/* `count` buffers cleared to zero, eight per launch (a launch per buffer costs the stream ~5 us whatever it moves): the
 * zero zones of a recorded step and the gradient slots its split-K products add into.  buffers[i] (a HOST array of
 * device pointers, as bytes is a host array) is 16-byte aligned and bytes[i] a multiple of 16. */
int cloudaae_zero_buffers(int count, void *const *buffers, const long long *bytes, cloudaae_stream_t stream);
/* :232-233  out[b,r,:] = x[b,r,:] + v[b,:] */
int cloudaae_add_rowvec(int b, int r, int d, const float *x, const float *v, float *out,
                        cloudaae_stream_t stream);
int cloudaae_add_f32(long long n, const float *a, const float *b, float *out, cloudaae_stream_t stream);
/* out = a + b*c elementwise (a may be NULL): the VAE reparameterisation, models/...:953 */
int cloudaae_mul_add_f32(long long n, const float *a, const float *b, const float *c, float *out,
                         cloudaae_stream_t stream);
/* get_edge_feature (utils/tf_util.py:635-669; with_center = 0: _wo_center, :672-706), unfused:
 * x[b*n, c] (row stride ldx), nn_idx[b,n,k] -> out[b,n,k,(1+with_center)*c]; and its gradient
 * (dx[b*n, c] is zero-filled here). */
int cloudaae_edge_feature(int b, int n, int k, int c, int with_center, const float *x, int ldx,
                          const int *nn_idx, float *out, cloudaae_stream_t stream);
int cloudaae_edge_feature_grad(int b, int n, int k, int c, int with_center, const float *g, const int *nn_idx,
                               float *dx, cloudaae_stream_t stream);
/* tf.reduce_mean (mode 1) / tf.reduce_max (mode 2) over groups of `rows` consecutive rows of
 * x[groups*rows, c] -> out[groups, c] (+ tie count for max), and the gradient. */
int cloudaae_pool_rows(int groups, int rows, int c, int mode, const float *x, float *out, float *ties,
                       cloudaae_stream_t stream);
int cloudaae_pool_rows_grad(int groups, int rows, int c, int mode, const float *x, const float *out,
                            const float *ties, const float *g, float *dx, cloudaae_stream_t stream);
/* out[i] = scalar[0] * scale (+ add[i]) : gradient of a mean */
int cloudaae_fill_scaled(long long n, const float *scalar, float scale, const float *add, float *out,
                         cloudaae_stream_t stream);
long long cloudaae_mean_workspace_bytes(void);
int cloudaae_mean_f32(long long n, const float *x, float *out, void *workspace, cloudaae_stream_t stream);
/* per[i] = a[i] + b[i] and out = mean(per) in one pass (chamfer_loss.py:13-14); workspace as for the mean. */
int cloudaae_add_mean_f32(long long n, const float *a, const float *b, float *per, float *out, void *workspace,
                          cloudaae_stream_t stream);
/* losses/trans_distance.py:4-9 */
int cloudaae_trans_error(int b, const float *pred, const float *label, float *per, cloudaae_stream_t stream);
int cloudaae_trans_error_grad(int b, const float *pred, const float *label, const float *per,
                              const float *gper, float *dpred, cloudaae_stream_t stream);
/* losses/angular_distance_taylor.py:30-116 in float64: per[b] = geodesic angle,
 * jac[b,3] = d per / d pred, loss = mean (fp32). */
int cloudaae_rotation_error(int b, const float *pred, const double *label, double *per, double *jac,
                            float *loss, cloudaae_stream_t stream);
/* exponential_map (angular_distance_taylor.py:30-66): axag[b,3] f64 -> rot[b,3,3] f64 */
int cloudaae_exponential_map(int b, const double *axag, double *rot, cloudaae_stream_t stream);
int cloudaae_rotation_error_grad(int b, const double *jac, const float *gloss, float *dpred,
                                 cloudaae_stream_t stream);
/* The whole loss tail of train_cloudAAE_ycbv.py:241-268 in one launch: translation error per sample
 * (trans_per[b]) and its mean, SO(3) geodesic error per sample in float64 (rot_per[b], with the
 * Jacobian rot_jac[b,3] w.r.t. rot_pred) and its mean, total = w_xyz*xyz_loss + w_trans*trans_loss +
 * w_rot*rot_loss.  Same arithmetic as cloudaae_trans_error / cloudaae_rotation_error /
 * cloudaae_loss_mix.  _grad: d(total) -> d(xyz_loss), d(trans_pred)[b,3], d(rot_pred)[b,3]. */
int cloudaae_pose_losses(int b, const float *trans_pred, const float *trans_label, const float *rot_pred,
                         const double *rot_label, const float *xyz_loss, float w_xyz, float w_trans, float w_rot,
                         float *trans_per, float *trans_loss, double *rot_per, double *rot_jac, float *rot_loss,
                         float *total, cloudaae_stream_t stream);
int cloudaae_pose_losses_grad(int b, const float *trans_pred, const float *trans_label, const float *trans_per,
                              const double *rot_jac, const float *g_total, float w_xyz, float w_trans,
                              float w_rot, float *d_xyz_loss, float *d_trans_pred, float *d_rot_pred,
                              cloudaae_stream_t stream);
/* The WHOLE loss tail in one launch: cloudaae_add_mean_f32 (per[n] = dist1 + dist2, xyz_loss = its mean, partial sums
 * in fixed order), then, in the workgroup that finishes last, cloudaae_pose_losses and -- g_total != NULL: the step's
 * upstream d(total) is known now -- cloudaae_pose_losses_grad; same arithmetic as those three.  g_total NULL: the three
 * gradient outputs are not touched and may be NULL.  workspace: cloudaae_loss_tail_workspace_bytes() bytes; ticket:
 * one int holding zero, left zero. */
long long cloudaae_loss_tail_workspace_bytes(void);
int cloudaae_loss_tail(long long n, const float *dist1, const float *dist2, float *per, float *xyz_loss, int b,
                       const float *trans_pred, const float *trans_label, const float *rot_pred,
                       const double *rot_label, float w_xyz, float w_trans, float w_rot, float *trans_per,
                       float *trans_loss, double *rot_per, double *rot_jac, float *rot_loss, float *total,
                       const float *g_total, float *d_xyz_loss, float *d_trans_pred, float *d_rot_pred,
                       void *workspace, int *ticket, cloudaae_stream_t stream);
/* :268  total = w0*a + w1*b + w2*c on device scalars */
int cloudaae_loss_mix(const float *a, const float *b, const float *c, float w0, float w1, float w2,
                      float *out, cloudaae_stream_t stream);
int cloudaae_loss_mix_grad(const float *g, float w0, float w1, float w2, float *ga, float *gb, float *gc,
                           cloudaae_stream_t stream);
/* :263-273  tf.train.AdamOptimizer (ApplyAdam form) over a flat buffer; beta powers are
 * device scalars (TF's beta1_power/beta2_power variables), multiplied when advance != 0. */
int cloudaae_adam_tf(long long n, float *param, const float *grad, float *m, float *v, float lr,
                     float beta1, float beta2, float eps, float *beta1_power, float *beta2_power,
                     float grad_scale, int advance, cloudaae_stream_t stream);
/* The same plus the end-of-step bookkeeping, done by the last workgroup of the kernel to finish: beta powers
 * advance, *step += step_inc (the `batch` counter, :192) and, if bn_decay != NULL, the batch-norm decay of the
 * NEXT step = min(bn_clip, 1 - bn_init * bn_rate^floor(step * batch_size / bn_decay_step)) (:194-202, what
 * cloudaae_bn_decay_schedule computes).  ticket: one int holding zero, left zero. */
int cloudaae_adam_tf_step(long long n, float *param, const float *grad, float *m, float *v, float lr, float beta1,
                          float beta2, float eps, float *beta1_power, float *beta2_power, float grad_scale,
                          float *step, float step_inc, float batch_size, float bn_init, float bn_decay_step,
                          float bn_rate, float bn_clip, float *bn_decay, int *ticket, cloudaae_stream_t stream);
int cloudaae_sgd(long long n, float *param, const float *grad, float lr, float grad_scale,
                 cloudaae_stream_t stream);
/* :194-202  out[0] = min(clip, 1 - init * rate^floor(step[0]*batch_size/decay_step)) */
int cloudaae_bn_decay_schedule(const float *step, float batch_size, float init, float decay_step,
                               float rate, float clip, float *out, cloudaae_stream_t stream);
int cloudaae_increment(float *x, float by, cloudaae_stream_t stream);

/* ---- on-line synthesis (train_cloudAAE_ycbv.py:79-117) ------------------------------------ */

/* transform_object_model (train...:88-93): out[b,j,:] = models[class_id[b], j, 0:3] R_b^T + t_b.
 * models [nmodels,npts,6] (xyz|rgb, obj_models.tfrecords), rot [b,3,3] f64 (cloudaae_exponential_map). */
int cloudaae_transform_object_model(int b, int npts, int nmodels, const float *models,
                                    const long long *class_id, const double *rot, const float *trans,
                                    float *out, cloudaae_stream_t stream);
/* get_random_spherical_occluder (utils/generate_occluder.py:38-81): two Gaussian blobs of per_blob
 * points (sigma), centres ~ N(0,wnear/10), N(0,hnear/10), N((near+z)/2,(z-near)/6), z = trans[:,2];
 * occluder [b, 2*per_blob, 3], blobs interleaved row by row as in the reference.  Counter-based RNG
 * (Philox4x32-10) keyed by `seed`: same distribution as tf.random.normal, not the same stream. */
int cloudaae_random_spherical_occluder(int b, int per_blob, const float *trans, float wnear, float hnear,
                                       float near_dist, float sigma, unsigned long long seed, float *occluder,
                                       cloudaae_stream_t stream);
/* Training poses drawn on the device (utils/sample_pose_in_frustum.py:8-153; DESIGN.md, "Pose sampling", has the
 * definition).  Sample i of the call is global sample g = first_index + i; every draw is a function of (seed, g, Philox
 * stream id) alone, so a sample does not depend on b, on the number of ranks or on the launch.
 *   classes [n_classes] int, HOST memory (read before the launch, passed by value): the class ids to draw from, each in
 *   [0, nmodels); NULL with n_classes = 0: every model.  At most 128 entries.
 *   wnear, wfar: the frustum widths of get_frustum; near_dist, far_dist; fx, fy, cx, cy, width, height: the camera.
 * Outputs (device): class_id [b] int64; axisangle [b,3] f64 (the fp32 axis * angle, widened); rot_mat64 [b,3,3] f64 =
 * cloudaae_exponential_map of it (the same bits); rot_mat32 [b,3,3] f32 = its rounding (optional); translation [b,3] f32: the draw when it projects strictly inside the
 * image, else the frustum middle (0, 0, (far+near)/2); in_fov [b] uint8: which of the two.  Optional (NULL to skip):
 * drawn [b,5] f32 = the draw before replacement and its pixel (x, y, z, u, v); raw [b,8] uint32 = the Philox words of
 * the pose and the translation stream.  One launch, no read-back; every argument is validated before any HIP call. */
int cloudaae_sample_poses(int b, unsigned long long first_index, unsigned long long seed, int n_classes,
                          const int *classes, int nmodels, float wnear, float wfar, float near_dist, float far_dist,
                          float fx, float fy, float cx, float cy, float width, float height, long long *class_id,
                          double *axisangle, double *rot_mat64, float *rot_mat32, float *translation,
                          unsigned char *in_fov, float *drawn, unsigned *raw, cloudaae_stream_t stream);
/* get_random_object_occluder (utils/generate_occluder.py:5-35): occluder [b,per,3] = the first `per` points of a class
 * model (models [nmodels,npts,6]) rotated by float32(rot_mat64[b]) -- the dot product of cloudaae_transform_object_model
 * -- plus a centre ~ N(0,wnear/8), N(0,hnear/8), N((near+z)/2,(z-near)/6), z = translation[:,2].  The class is drawn
 * PER SAMPLE from `classes` (HOST memory, as above; the reference draws one per process).  first_index and seed as
 * above, with stream ids of its own.  Optional: occ_class [b] int64, raw [b,8] uint32 (centre and class streams).
 * Every argument is validated before any HIP call; per <= npts. */
int cloudaae_random_object_occluder(int b, unsigned long long first_index, unsigned long long seed, int nmodels, int npts,
                                    const float *models, int n_classes, const int *classes, const double *rot_mat64,
                                    const float *translation, int per, float wnear, float hnear, float near_dist,
                                    float *occluder, long long *occ_class, unsigned *raw, cloudaae_stream_t stream);
/* sphericalFlip (utils/hidden_point_removal.py:6-24, 51-68): points = concat(a[b,na,3], bpts[b,nb,3])
 * - center; flipped = 2 (R - |p|) p / |p| + p, R = max|p| * 10^param; both outputs are
 * [b, na+nb+1, 3] with a zero last row (the viewpoint).  bpts may be NULL with nb = 0. */
int cloudaae_spherical_flip(int b, int na, const float *a, int nb, const float *bpts, const float *center,
                            float param, float *flipped, float *org, cloudaae_stream_t stream);
/* convexHull / hidden_point_removal (utils/hidden_point_removal.py:27-48): visible points = vertices of
 * conv(flipped[b,n1,3]) minus the two largest vertex indices (the reference's two `[:-1]`); visible
 * [b,n1,3] = org rows of the visible ids (ascending), padded with random re-draws of visible ids;
 * num_vis [b] int64; visible_id [b,n1] (optional; -1 in the padded rows).  qhull is replaced by an exact
 * per-point vertex test (2-variable LPs in fp64: a local problem over the point's neighbours in a spatial
 * order, then verification passes over bounding volumes of 64-point groups; the points of a cloud are handed
 * to waves from a per-cloud queue); workspace: cloudaae_hpr_workspace_bytes(b, n1) (vertex flags, the sorted
 * cloud, its permutation, the queues -- contents undefined afterwards).  The points of a cloud are taken to be
 * distinct (qhull reports one of several identical vertices; here an exact copy of a binding constraint tests
 * as violated by round-off and the answer for such points is unspecified). */
long long cloudaae_hpr_workspace_bytes(int b, int n1);
int cloudaae_hidden_point_removal(int b, int n1, const float *flipped, const float *org,
                                  unsigned long long seed, float *visible, long long *num_vis, int *visible_id,
                                  void *workspace, cloudaae_stream_t stream);
/* The same with a chosen number of output rows: visible [b,rows,3] (visible_id [b,rows]) = the visible points in
 * ascending index, then random re-draws of visible points up to `rows` rows -- the reference's rule
 * (hidden_point_removal.py:38-40, where rows == n1) for a Chamfer target of 4N rows when 4N exceeds the model's
 * point count (BASELINE configs[4]: N = 4096).  row_src [b,rows] (optional): for every output row the row < num_vis it
 * is equal to (itself for the visible points, the drawn one for a re-draw; -1 when nothing is visible) -- what
 * cloudaae_nn_distance_prefix needs to search the distinct target points only. */
int cloudaae_hidden_point_removal_rows(int b, int n1, const float *flipped, const float *org,
                                       unsigned long long seed, int rows, float *visible, long long *num_vis,
                                       int *visible_id, int *row_src, void *workspace, cloudaae_stream_t stream);

/* ---- pose refinement: point-to-point ICP (evaluate_cloudAAE_ycbv.py:606-628) ---- */

/* Batched point-to-point ICP with open3d's registration_icp semantics (TransformationEstimationPointToPoint without
 * scaling), run as a schedule of `rounds` calls whose correspondence radius starts at `radius` and is multiplied by
 * `decay` after each call; each call starts from the previous call's transform and stops after max_iteration updates
 * or when |d fitness| < relative_fitness and |d rmse| < relative_rmse.  All arithmetic is float64 ("Pose
 * refinement", has the definition).  Per cloud c:
 *   src: m points (x, y, z) at src + c*src_cloud_stride + i*src_point_stride (the object model, object frame);
 *   dst: n points likewise (the scene, camera frame); strides in floats, >= 3 per point;
 *   rot_axag [b,3], trans [b,3]: the initial pose (axis-angle, Rodrigues; a zero vector is the identity);
 *   transform [b,4,4] f64 row-major (last row 0 0 0 1), rot_out [b,3] f64 (axis-angle of the result, angle in
 *   [0, pi]), trans_out [b,3] f32 (its translation), fitness [b] and rmse [b] f64 of the last round,
 *   iterations [b,rounds] int (updates performed in each round; may be NULL when rounds == 0).
 * rounds == 0 returns the initial transform with the statistics of its correspondences at `radius`.
 * Limits: 1 <= m <= 4096, 1 <= n <= 4096 (CLOUDAAE_ICP_MAX_POINTS), rounds >= 0, max_iteration >= 0, radius > 0,
 * 0 < decay <= 1.  The result of a cloud does not depend on the rest of the batch and is bit-reproducible. */
#define CLOUDAAE_ICP_MAX_POINTS 4096
int cloudaae_icp_point_to_point(int b, int m, const float *src, int src_point_stride, long long src_cloud_stride,
                                int n, const float *dst, int dst_point_stride, long long dst_cloud_stride,
                                const float *rot_axag, const float *trans, double radius, double decay, int rounds,
                                int max_iteration, double relative_fitness, double relative_rmse,
                                double *transform, double *rot_out, float *trans_out, double *fitness,
                                double *rmse, int *iterations, cloudaae_stream_t stream);
/* The same schedule, matching, tie rule, statistics (fitness, Euclidean inlier rmse), stopping rule and outputs with
 * the point-to-plane update ("Pose refinement", has the definition): with p the transformed source point, q
 * its target point and n = tgt_normals[c, j] that point's normal, r = (p - q) . n, J = [p x n; n], A = sum J J^T,
 * b = sum J r, A x = -b by LDL^T in float64, x = (alpha, beta, gamma, t), U = [Rz(gamma) Ry(beta) Rx(alpha) | t].  Fewer
 * than six correspondences, a pivot that is not a finite number > 0 or a solution that is not finite leave the pose as
 * it is.  tgt_normals [b,n,3] float64, packed, one per target point (their sign does not matter).
 * pose_maps_target_to_source != 0: rot_axag / trans and every returned pose (transform, rot_out, trans_out) are the
 * target -> source pose: the kernel inverts the initial pose on entry (R^T, -R^T t) and the result on exit, so a caller
 * holding model -> camera poses can run the iteration scene -> model (src = the scene, dst = the model with its
 * normals).  fitness and rmse are always those of the src points.  Limits as above. */
int cloudaae_icp_point_to_plane(int b, int m, const float *src, int src_point_stride, long long src_cloud_stride,
                                int n, const float *dst, int dst_point_stride, long long dst_cloud_stride,
                                const double *tgt_normals, int pose_maps_target_to_source, const float *rot_axag,
                                const float *trans, double radius, double decay, int rounds, int max_iteration,
                                double relative_fitness, double relative_rmse, double *transform, double *rot_out,
                                float *trans_out, double *fitness, double *rmse, int *iterations,
                                cloudaae_stream_t stream);
/* y[i] = (float)x[i], round to nearest even (an f64 result handed to an fp32 consumer, e.g. a loss kernel). */
int cloudaae_f64_to_f32(long long n, const double *x, float *y, cloudaae_stream_t stream);

/* ---- surface normals ("Surface normals", has the definition) ---- */

/* Normals of k query points per set from the covariance of their radius neighbourhood in the set's support points.
 *   support: s packed sets, set i = the points offsets[i] .. offsets[i+1] (offsets [s+1] int, device) of xyz, point j
 *   at xyz + j*xyz_point_stride (floats, >= 3: obj_batch [b,2048,6] goes in unsliced), max_points points in all;
 *   queries: k per set, query i of set c at queries + c*query_set_stride + i*query_point_stride (may be the support).
 * Neighbours of a query: the support points of its set with ((dx^2 + dy^2) + dz^2) < r^2 in double on the widened
 * coordinates, r = (double)radius.  count [s,k] = their number.  count < min_neighbors: normal (0, 0, 1), eigenvalues
 * 0.  Otherwise the covariance about the neighbours' mean (two passes, float64, divided by count), its eigenvalues in
 * ascending order -> eigenvalues [s,k,3] and the unit eigenvector of the smallest -> normals [s,k,3] (cyclic Jacobi).
 * viewpoint (HOST pointer to three doubles, read during the call; NULL = none): an estimated normal is flipped when
 * n . (q - v) > 0; without one its sign is the solver's.  Two launches, no floating-point atomics; a set's result does
 * not depend on s and is bit-reproducible.  workspace: cloudaae_estimate_normals_workspace_bytes(s, max_points) bytes
 * (-1 for a bad argument).  Limits: 1 <= s <= 65535, k >= 1, s*k <= 2^30, 1 <= max_points <= 2^28, radius > 0,
 * min_neighbors >= 3. */
long long cloudaae_estimate_normals_workspace_bytes(int s, long long max_points);
int cloudaae_estimate_normals(int s, const int *offsets, const float *xyz, int xyz_point_stride, long long max_points,
                              int k, const float *queries, int query_point_stride, long long query_set_stride,
                              float radius, int min_neighbors, const double *viewpoint, double *normals,
                              double *eigenvalues, int *count, void *workspace, long long workspace_bytes,
                              cloudaae_stream_t stream);

/* ---- pose scores: ADD, ADD-S, model diameter ("Pose scores", has the definition) ---- */

/* ADD and ADD-S of p estimated poses per sample against the sample's ground truth, in float64 on the exactly promoted
 * float32 model.  Per sample s:
 *   model: m points (x, y, z) at model + s*cloud_stride + i*point_stride (strides in floats, >= 3 per point: obj_batch
 *   [b,2048,6] goes in unsliced); est [b,p,4,4] and gt [b,4,4] float64 row-major (only the top three rows are read).
 * With g_i = gt x_i and e_i = est x_i (((R00 x + R01 y) + R02 z) + t0 row by row, no fma):
 *   add [b,p]  = (1/m) sum_i |g_i - e_i|;
 *   nn_d2 [b,p,m] (optional, may be NULL) = min_j |g_i - e_j|^2, |d|^2 = (dx^2 + dy^2) + dz^2;
 *   adds [b,p] = (1/m) sum_i sqrt(nn_d2[i]).
 * Both sums: blocks of 64 consecutive points, each added as a binary tree (halves folded: 64 -> 32 -> ... -> 1), the
 * blocks' sums added in ascending order.  Exact fp64 brute force over ceil(m/64) workgroups per sample and pose plus a
 * one-lane-per-result finishing launch; no floating-point atomics: the result does not depend on b, p or the run.
 * workspace: cloudaae_pose_score_workspace_bytes(b, p, m) bytes (-1 for a bad argument), need not be initialised.
 * Limits: b, p, m >= 1; b * p * ceil(m/64) <= 2^31 - 1. */
long long cloudaae_pose_score_workspace_bytes(int b, int p, int m);
int cloudaae_pose_score(int b, int p, int m, const float *model, int point_stride, long long cloud_stride,
                        const double *est, const double *gt, double *add, double *adds, double *nn_d2,
                        void *workspace, cloudaae_stream_t stream);
/* T0 of "Pose refinement": out [b,4,4] float64 row-major = [Rodrigues(rot) | trans; 0 0 0 1] from an axis-angle
 * rot [b,3], float32 (rot_is_f64 = 0: the network's) or float64 (rot_is_f64 = 1: the ground truth's), and a float32
 * translation [b,3].  A zero rot gives the identity rotation. */
int cloudaae_pose_matrix(int b, const void *rot, int rot_is_f64, const float *trans, double *out,
                         cloudaae_stream_t stream);
/* out [b,2,4,4] = (first [b,4,4], second [b,4,4]) sample by sample: two pose sets as the est of one
 * cloudaae_pose_score launch with p = 2. */
int cloudaae_pose_stack(int b, const double *first, const double *second, double *out, cloudaae_stream_t stream);
/* diam [c] float64 = sqrt(max_{i<j} ((dx^2 + dy^2) + dz^2)) over the m points of each of c clouds (0 for m = 1), read
 * with strides as above.  The same tile loop as cloudaae_pose_score with max in place of min; max is exact, so no order
 * matters.  workspace: cloudaae_cloud_diameter_workspace_bytes(c, m) bytes.  Limit: c * ceil(m/64) <= 2^31 - 1. */
long long cloudaae_cloud_diameter_workspace_bytes(int c, int m);
int cloudaae_cloud_diameter(int c, int m, const float *model, int point_stride, long long cloud_stride, double *diam,
                            void *workspace, cloudaae_stream_t stream);

/* ---- evaluation inputs from RGB-D frames (evaluate_cloudAAE_ycbv.py:164-271) ---- */

/* The segments of F frames, as the reference's evaluation cuts them ("Frame segments", has the definition):
 *   depth [f,h,w] uint16, label [f,h,w] uint8 (class + 1; 0 = none), intrinsics [f,5] float (fx, fy, cx, cy,
 *   factor_depth); segment i is class seg_class[i] (0-based) of frame seg_frame[i] (a pair named twice: only its last
 *   segment gets the points, the others are empty).
 * Per segment: the pixels whose label - 1 is the class and whose depth is not 0, back-projected in fp32; their mean
 * (the fp64 sum in pixel order / count, rounded to fp32) -> mean [s,3]; the points within `threshold` of it, in pixel
 * order, packed segment after segment -> xyz [f*h*w, 3] at offsets[i] .. offsets[i+1] (offsets [s+1] int, device;
 * num_point_after_filter = the difference).  workspace: cloudaae_frame_segments_workspace_bytes(f, h, w, s) bytes.
 * Limits: f*h*w <= 2^28.  A memset and ten launches; bit-reproducible; a segment's result does not depend on the batch. */
long long cloudaae_frame_segments_workspace_bytes(int f, int h, int w, int s);
int cloudaae_frame_segments(int f, int h, int w, const uint16_t *depth, const uint8_t *label, const float *intrinsics,
                            int s, const int *seg_frame, const int *seg_class, float threshold, int *offsets,
                            float *xyz, float *mean, void *workspace, long long workspace_bytes,
                            cloudaae_stream_t stream);
/* open3d's remove_radius_outlier(nb_points, radius) on each of s packed point sets (offsets [s+1] device, the points
 * at xyz, at most max_points in all): point j keeps when more than nb_points points of its set (itself included) lie
 * at d^2 < r^2, d^2 = ((dx^2 + dy^2) + dz^2) in double and r = (double)radius.  A set with fewer than min_keep
 * keepers keeps all its points.  Outputs: in_offsets [s+1], in_index [max_points] (each inlier's index within its
 * set), in_xyz [max_points,3] (packed like the input), num_valid [s] = the inliers whose index is not 0 (numpy's
 * count_nonzero of the index list, :280).  workspace: cloudaae_radius_outlier_workspace_bytes(s, max_points). */
long long cloudaae_radius_outlier_workspace_bytes(int s, long long max_points);
int cloudaae_radius_outlier(int s, const int *offsets, const float *xyz, long long max_points, int nb_points,
                            float radius, int min_keep, int *in_offsets, int *in_index, float *in_xyz, int *num_valid,
                            void *workspace, long long workspace_bytes, cloudaae_stream_t stream);
/* FPS_random of the reference (:226-247) on each of s packed point sets, from starts[i] (device): idx[i,0] = start;
 * idx[i,j] = the first index of the largest dist, then dist = min(dist, d(idx[i,j])), with
 * d = (dx^2 + dy^2) + dz^2 in double on the widened coordinates; out_xyz [s,k,3] = the points picked.  k may exceed
 * the set's size (the picks then repeat index 0 once every distance is 0).  A set that is empty or whose start lies
 * outside [0, n) gives idx -1 and zeros.  workspace: cloudaae_ragged_fps_workspace_bytes(max_points). */
long long cloudaae_ragged_fps_workspace_bytes(long long max_points);
int cloudaae_ragged_fps(int s, const int *offsets, const float *xyz, long long max_points, int k, const int *starts,
                        int *idx, float *out_xyz, void *workspace, long long workspace_bytes,
                        cloudaae_stream_t stream);

/* ---- object models from triangle meshes ("Mesh sampling", has the definition) ---- */

/* s packed meshes: mesh i owns the vertices vert_offsets[i] .. vert_offsets[i+1] of vertices [num_vertices,3] f32 (and
 * of colors, where given) and the triangles tri_offsets[i] .. tri_offsets[i+1] of triangles [num_triangles,3] int,
 * whose indices are local to the mesh (offsets [s+1] int, device).  A mesh whose offsets do not lie inside the packed
 * arrays counts as empty.  At most 2^24 triangles per mesh; s <= 65535; num_vertices, num_triangles <= 2^28.
 *
 * Weights: in double on the widened coordinates, no fma: n = (b - a) x (c - a), each component (p q) - (r s);
 * A2 = sqrt((nx^2 + ny^2) + nz^2); a2max [s] f64 = the largest of the mesh (an integer maximum on the bit pattern: exact
 * in any order; 0 for a mesh without a valid triangle); weights [num_triangles] uint64 = floor(A2 / A2max * 2^32), in
 * [0, 2^32].  A triangle with a vertex index outside its mesh, or whose A2 is not finite or is 0, gets weight 0 and is
 * counted in invalid [s].  A triangle below 2^-32 of the mesh's largest gets weight 0 as well (it is never drawn) and is
 * not counted.  cum [num_triangles] uint64 = the inclusive prefix sum of the weights inside each mesh (integer, exact).
 * A memset and four launches, no floating-point atomic, no read-back.  workspace:
 * cloudaae_mesh_weights_workspace_bytes(num_triangles) bytes (-1 for a bad argument), need not be initialised. */
long long cloudaae_mesh_weights_workspace_bytes(long long num_triangles);
int cloudaae_mesh_weights(int s, const int *vert_offsets, const int *tri_offsets, long long num_vertices,
                          long long num_triangles, const float *vertices, const int *triangles,
                          unsigned long long *weights, unsigned long long *cum, double *a2max, int *invalid,
                          void *workspace, long long workspace_bytes, cloudaae_stream_t stream);
/* n area-uniform surface samples of every mesh, by the cumulative weights `cum` (those of cloudaae_mesh_weights, or the
 * caller's own: non-decreasing inside a mesh).  Sample j of mesh i has the global index g = first_index + j (< 2^40) and
 * the four words r of philox4x32(seed, id * 2^40 + g, stream 20), id = mesh_ids[i] (device, [s]; NULL: id = i):
 * with W = the mesh's last cum, target = the high 64 bits of (r0 2^32 + r1) W; the triangle is the first t with
 * cum[t] > target; u = u01(r2), v = u01(r3) widened, both replaced by 1 - u, 1 - v when u + v > 1; b0 = (1 - u) - v;
 * p = (b0 a + u b) + v c per coordinate in double, rounded once to float.  colors [num_vertices,3] f32 (NULL: zeros) are
 * mixed the same way.  Outputs: xyzrgb [s,n,6] f32; tri [s,n] int (local to the mesh); normal [s,n,3] f64 (optional) =
 * n / A2 of the triangle, its sign the winding's.  A mesh with W = 0, and a draw whose triangle has an index outside
 * its mesh (possible with the caller's own cum only), give zeros and triangle -1.  One launch, one lane per sample; a
 * sample does not depend on s, n or the launch.  Limits as above; s * n <= 2^28. */
int cloudaae_mesh_sample(int s, const int *vert_offsets, const int *tri_offsets, long long num_vertices,
                         long long num_triangles, const float *vertices, const float *colors, const int *triangles,
                         const unsigned long long *cum, const int *mesh_ids, int n, unsigned long long first_index,
                         unsigned long long seed, float *xyzrgb, int *tri, double *normal, cloudaae_stream_t stream);
/* dst[i, j, 0..cols) = src[i, idx[i, j], 0..cols) for s sets of rows_per_set rows: idx [s,k] int (device) is local to
 * the set, as cloudaae_ragged_fps returns it (outside [0, rows_per_set): a row of zeros); NULL: row j itself
 * (k <= rows_per_set), which repacks a column range.  Row r of the source starts at src + r * src_row_stride elements,
 * of the destination at dst + r * dst_row_stride (both >= cols); elem_bytes is 4 or 8.  s * k * cols <= 2^32. */
int cloudaae_mesh_gather_rows(int s, int k, const int *idx, long long rows_per_set, const void *src,
                              long long src_row_stride, int cols, int elem_bytes, void *dst, long long dst_row_stride,
                              cloudaae_stream_t stream);

/* ---- depth and label frames of posed meshes ("Rendered frames", has the definition) ---- */

/* f frames of h x w from j posed instances of the s packed meshes above (the layout of cloudaae_mesh_weights):
 *   intrinsics [f,5] float (fx, fy, cx, cy, factor_depth: the rows cloudaae_frame_segments takes); the instances of
 *   frame i are inst_offsets[i] .. inst_offsets[i+1] (inst_offsets [f+1] int); instance i draws mesh inst_mesh[i] under
 *   the pose inst_pose[i] ([j,16] double, row-major 4x4, top three rows read: what cloudaae_pose_matrix writes) and
 *   writes inst_label[i] (1..255; only the low 8 bits are kept) into `label`.
 *   inst_vert_base, inst_tri_base [j+1] int: the exclusive prefix sums of the instances' vertex and triangle counts
 *   in instance order, computed by the host from its copies of the offsets; sum_inst_vertices and sum_inst_triangles
 *   are their last entries.  The draw rank of triangle t of instance i is inst_tri_base[i] + t.  All arrays are device
 *   memory.  An instance whose mesh id or offsets do not describe ranges inside the packed arrays, or that lies in no
 *   frame, draws nothing; bases that do not fit the meshes misplace ranks but never an access.
 * Vertices: p = pose x in double on the widened floats (((R00 x + R01 y) + R02 z) + t0, no fma); sx = (fx X) / Z + cx,
 * ix = floor(256 sx + 0.5), likewise iy; unusable when Z is not finite, Z < z_near or |ix|, |iy| > 2^24.  A triangle
 * with an unusable vertex or an index outside its mesh is counted in dropped [j], one of zero fixed-point area in
 * degenerate [j]; there is no clipping and no culling.  Pixel (u, v) is sampled at (256 u, 256 v); it is covered when
 * the three int64 edge values w are >= 0; its depth is z = area2 / ((w_a / Z_a + w_b / Z_b) + w_c / Z_c) and
 * du = floor(z factor_depth + 0.5), kept when 1 <= du <= 65535; the pixel takes the minimum of (du << 32 | rank).
 * Outputs: depth [f,h,w] uint16 (0: nothing drawn), label [f,h,w] uint8 (0: background), tri [f,h,w] int (optional:
 * the winning rank, -1 where empty), dropped, degenerate [j] int.  Every output is an integer and does not depend on
 * the order of execution, the batch or the run.  Four memsets and four launches (vertices; setup, which rasterises
 * the triangles of at most 16 samples and queues the others; the queue, one wave per triangle; resolve); only integer
 * atomics; no read-back.  workspace: cloudaae_render_workspace_bytes(...) bytes, need not be initialised; the query
 * returns 0 outside the limits, and the launch then returns an error without launching.  Limits: f, h, w, j >= 1;
 * h * w <= 2^24; f * h * w <= 2^28; sum_inst_vertices, sum_inst_triangles < 2^31; at most 2^24 triangles per mesh
 * (checked as sum_inst_triangles <= j * 2^24); z_near > 0. */
long long cloudaae_render_workspace_bytes(int f, int h, int w, int j, long long sum_inst_vertices,
                                          long long sum_inst_triangles);
int cloudaae_render_frames(int s, const int *vert_offsets, const int *tri_offsets, long long num_vertices,
                           long long num_triangles, const float *vertices, const int *triangles, int f, int h, int w,
                           const float *intrinsics, const int *inst_offsets, int j, const int *inst_mesh,
                           const int *inst_label, const double *inst_pose, const int *inst_vert_base,
                           const int *inst_tri_base, long long sum_inst_vertices, long long sum_inst_triangles,
                           double z_near, uint16_t *depth, uint8_t *label, int *tri, int *dropped, int *degenerate,
                           void *workspace, long long workspace_bytes, cloudaae_stream_t stream);

/* ---- BOP pose errors ("BOP pose errors (VSD, MSSD, MSPD)", has the definition) ---- */

/* The pixel counts behind the visible surface discrepancy of b samples with p estimated poses each.
 *   depth_test [f,h,w] uint16 with intrinsics [f,5] float (fx, fy, cx, cy, factor_depth); frame_of [b] int: the test
 *   frame of each sample; depth_gt [b,h,w], depth_est [b,p,h,w] uint16: the object's mesh alone, rendered with that
 *   frame's intrinsics under the ground truth and under the estimates; tau [b,k] double.  All device memory.
 * Per pixel (u = column, v = row), in double, no fma: m = sqrt((xn xn + yn yn) + 1) with xn = (u - cx) / fx,
 * yn = (v - cy) / fy; D(d) = (d / factor) m; valid_t = dt != 0; vis_g = dg != 0 and (not valid_t or D(dg) - D(dt) <=
 * delta); vis_e = de != 0 and (not valid_t or D(de) - D(dt) <= delta or vis_g).
 * Outputs (int, zeroed by the call): inter [b,p] = #(vis_g and vis_e); uni [b,p] = #(vis_g or vis_e); over [b,p,k] =
 * #(vis_g and vis_e and |D(dg) - D(de)| >= tau[k]); visib_gt [b] = #vis_g.  Four memsets and one launch; integer atomics
 * only, so the counts do not depend on the order of execution, the batch or the run.  A frame_of entry outside [0, f)
 * leaves that sample's counts 0 and causes no access.  Limits: f, h, w, b, p >= 1; 1 <= k <= 16; h * w <= 2^24;
 * b * p * h * w <= 2^28; outside them the call returns an error and launches nothing. */
int cloudaae_vsd_counts(int f, int h, int w, const uint16_t *depth_test, const float *intrinsics, int b, int p,
                        const int *frame_of, const uint16_t *depth_gt, const uint16_t *depth_est, double delta, int k,
                        const double *tau, int *inter, int *uni, int *over, int *visib_gt, cloudaae_stream_t stream);

/* MSSD and MSPD of b samples with p estimated poses each on the model points of cloudaae_pose_score (model, point_stride,
 * cloud_stride, est [b,p,16], gt [b,16] as there).  sym [b,smax,16] double: the symmetry transforms of each sample's
 * object (row-major 4x4, top three rows read), of which the first num_sym[b] (clamped into 1..smax) are used; the
 * identity must be among them.  mssd [b,p] = min_s sqrt(max_i |E x_i - G (S_s x_i)|^2), squares summed as (dx^2 + dy^2)
 * + dz^2.  intrinsics [b,5] float (each sample's frame) and mspd [b,p] go together, both or NULL: mspd = min_s
 * sqrt(max_i ((ue - ug)^2 + (ve - vg)^2)) with u = (fx X) / Z + cx, v = (fy Y) / Z + cy, and +inf when a Z under E or
 * G S_s is not > 0.  Maxima and minima are exact (integer comparisons on the bit patterns); a memset and two launches.
 * workspace: cloudaae_pose_max_dist_workspace_bytes(b, p, smax) bytes (-1 for an argument below 1), need not be
 * initialised.  Limits: b * p * ceil(m / 128) < 2^31, b * p * smax <= 2^28. */
long long cloudaae_pose_max_dist_workspace_bytes(int b, int p, int smax);
int cloudaae_pose_max_dist(int b, int p, int m, const float *model, int point_stride, long long cloud_stride,
                           const double *est, const double *gt, int smax, const int *num_sym, const double *sym,
                           const float *intrinsics, double *mssd, double *mspd, void *workspace, cloudaae_stream_t stream);

/* ---- a depth sensor's noise on depth / label frames ("Sensor noise", has the definition) ---- */

/* The slope at every pixel of f frames of h x w: depth [f,h,w] uint16 and label [f,h,w] uint8 as cloudaae_render_frames
 * writes them, intrinsics [f,5] float (fx, fy, cx, cy, factor_depth).  All device memory.  In double, no fma:
 * P(u, v) = (((u - cx) dm) / fx, ((v - cy) dm) / fy, dm), dm = d / factor_depth.  A neighbour is valid inside the image
 * with depth != 0 and the pixel's label; along each axis the central difference P(+1) - P(-1), else the one-sided
 * difference with the valid neighbour, else none.  A pixel with depth is flat (normal zeros, theta 0) when an axis has no
 * difference or n = gx x gy has n . n = 0 or not finite; otherwise theta = acos(min(|n . ray| / (sqrt(n . n) sqrt(ray .
 * ray)), 1)) with ray = P of the pixel, and the normal is n / sqrt(n . n) turned so that n . ray <= 0.
 * Outputs: normals [f,h,w,3] float, theta [f,h,w] float (optional, may be NULL), both zeros where depth is 0;
 * flat_counts [f] int (zeroed by the call): the flat pixels among those with depth.  A memset and one launch, integer
 * atomics only.  Limits: f, h, w >= 1; h * w <= 2^24; f * h * w <= 2^28; outside them, or with a null pointer, the call
 * returns an error and launches nothing. */
int cloudaae_depth_normals(int f, int h, int w, const uint16_t *depth, const uint8_t *label, const float *intrinsics,
                           float *normals, float *theta, int *flat_counts, cloudaae_stream_t stream);

/* The sensor model on the same inputs; frame i of the launch has the global index first_frame + i (below 2^40).  Per
 * destination pixel p = v w + u: (n_u, n_v) = normal2(r0, r1), (n_z, unused) = normal2(r2, r3) of philox4x32(seed,
 * (first_frame + i) 2^24 + p, 21), the dropout word r0 of stream 22; floats widened to double, all later arithmetic in
 * double without fma.  1. the source s = (clamp(u + rint(n_u sigma_l), 0, w - 1), clamp(v + rint(n_v sigma_l), 0, h - 1));
 * label_out = label(s); depth(s) = 0 gives depth 0.  2. z = dm(s), theta = min(slope at s, theta_max), sigma_z =
 * (a0 + a1 ((z - z0)(z - z0))) + ((a2 / sqrt(z)) (theta theta)) / ((pi/2 - theta)(pi/2 - theta)), z' = z + n_z sigma_z.
 * 3. depth 0 when the unclamped theta > theta_drop, else when r0 < floor(p_drop 2^32).  4. with disparity_step > 0:
 * k = rint(((fx baseline) / z') / disparity_step), k < 1 (or not a number) gives depth 0, z'' = (fx baseline) /
 * (k disparity_step); else z'' = z'.  5. du = floor(z'' factor_depth + 0.5), depth 0 unless 1 <= du <= 65535.
 * Outputs: depth_out [f,h,w] uint16, label_out [f,h,w] uint8 (neither may alias an input), counts [f,4] int (zeroed by
 * the call): destination pixels whose own input depth is not 0; pixels dropped by the angle; by chance; lost in steps 4
 * and 5 (each pixel with a source depth ends in exactly one of: kept, angle, chance, lost); z_noisy [f,h,w] double
 * (optional, may be NULL): z' where the source has depth and z' is finite, else 0.  A memset and one launch, integer
 * atomics only; the same (seed, global frame, p) gives the same pixel whatever f or the launch split.  Errors (nothing is
 * launched): the limits of cloudaae_depth_normals; first_frame + f > 2^40; sigma_l < 0; theta_max outside [0, pi/2);
 * p_drop outside [0, 1]; disparity_step < 0; a non-finite parameter; a null pointer.  factor_depth lives in device
 * memory and is not read by the host: a frame whose factor_depth is not > 0 comes out with depth 0 everywhere. */
int cloudaae_depth_sensor_noise(int f, int h, int w, const uint16_t *depth, const uint8_t *label, const float *intrinsics,
                                unsigned long long seed, unsigned long long first_frame, double sigma_l, double a0, double a1,
                                double z0, double a2, double theta_max, double theta_drop, double p_drop, double baseline,
                                double disparity_step, uint16_t *depth_out, uint8_t *label_out, int *counts, double *z_noisy,
                                cloudaae_stream_t stream);

/* ---- rendered training clouds ("Rendered training clouds", has the definition) ---- */

/* c fixed-size clouds of `rows` points from the labelled pixels of f frames of h x w: depth [f,h,w] uint16, label [f,h,w]
 * uint8, intrinsics [f,5] float as above.  Cloud i is described by frame_of[i] (int: the frame it reads), want[i] (int:
 * the label value that selects pixels) and index[i] (long long: its global index g, in [0, 2^39)); fallback [c,3] float
 * is optional (NULL: zeros).  All device memory, nothing is read back.
 * Mask: the pixels p = v w + u of the frame with label == want and depth != 0, n of them; the rank of a masked pixel is
 * its position among them in pixel order.  A masked pixel becomes the point (((u - cx) dm) / fx, ((v - cy) dm) / fy, dm),
 * dm = (float)depth / factor_depth, in float without fma (the back-projection of cloudaae_frame_segments).
 * q_j = word 0 of philox4x32(seed, g 2^24 + j, stream), stream 23 for n >= rows and 24 for n < rows.
 * n >= rows: with s_j = floor(j n / rows), row j is the masked pixel of rank s_j + floor(q_j (s_{j+1} - s_j) / 2^32):
 * one pixel per stratum, in pixel order, none twice; num_distinct = rows, row_src[j] = j.
 * 1 <= n < rows: rows 0 .. n-1 are the masked pixels in pixel order, row j >= n is a copy of row floor(q_j n / 2^32);
 * num_distinct = n, row_src[j] = j below n and the copied row above -- the (cloud, count, source) convention that
 * cloudaae_nn_distance_prefix takes.  n = 0: every row is fallback[i], num_distinct = 1, row_src = 0.
 * A cloud whose frame_of lies outside [0, f) or whose index lies outside [0, 2^39) is the n = 0 case and no frame is
 * read for it.
 * Outputs: cloud [c,rows,3] float, num_pixels [c] int (n), num_distinct [c] long long, row_src [c,rows] int.
 * Four launches; no atomic, nothing waits on another workgroup, and the same (frame bytes, want, seed, g) gives the same
 * cloud whatever c, f or the position in either.  workspace: cloudaae_frame_clouds_workspace_bytes bytes, which is 0
 * outside the limits: f, h, w, c >= 1; h * w <= 2^24; f * h * w <= 2^28; 1 <= rows <= 2^20; c * rows and
 * c * ceil(h w / 1024) below 2^31.  Outside them, with a null pointer or a small workspace, the call returns an error
 * and launches nothing. */
long long cloudaae_frame_clouds_workspace_bytes(int f, int h, int w, int c, int rows);
int cloudaae_frame_clouds(int f, int h, int w, const uint16_t *depth, const uint8_t *label, const float *intrinsics, int c,
                          const int *frame_of, const int *want, const long long *index, const float *fallback, int rows,
                          unsigned long long seed, float *cloud, int *num_pixels, long long *num_distinct, int *row_src,
                          void *workspace, long long workspace_bytes, cloudaae_stream_t stream);

/* The scene of a rendered training batch, assembled on the device as cloudaae_render_frames takes it: sample i of b
 * (global sample first_index + i) gives frame 2i with instance 3i -- mesh mesh_index[class_id[i]], label 1, pose
 * [rot_mat64[i] | translation[i]] -- and frame 2i + 1 with instance 3i + 1 (the same) and 3i + 2, the occluder: label 2,
 * mesh mesh_index[class], pose [rot_mat64[i] | centre], class and centre by the rule of cloudaae_random_object_occluder
 * (streams 19 and 18 under `seed`; classes / n_classes / nmodels, wnear, hnear, near_dist as there).  class_id [b] long
 * long, mesh_index [nmodels] int, rot_mat64 [b,9] double and translation [b,3] float are device memory; a class_id
 * outside [0, nmodels) gives mesh -1, which the renderer draws nothing for.  The classes are not known to the host, so
 * instance j's ranks start at j max_vertices and j max_triangles (the largest mesh's counts; the renderer treats ranks
 * past a mesh's own counts as absent): pass the sums 3 b max_vertices and 3 b max_triangles on.
 * Outputs (device): inst_offsets [2b+1], inst_mesh, inst_label [3b] int, inst_pose [3b,16] double, inst_vert_base,
 * inst_tri_base [3b+1] int, occ_class [b] long long, occ_centre [b,3] float (optional, may be NULL).  One launch.
 * Errors: b < 1; a maximum < 1; 3 b max_vertices or 3 b max_triangles above 2^31 - 1; a bad class list; a null pointer. */
int cloudaae_rendered_scene(int b, unsigned long long first_index, unsigned long long seed, int nmodels, int n_classes,
                            const int *classes, const long long *class_id, const int *mesh_index, const double *rot_mat64,
                            const float *translation, float wnear, float hnear, float near_dist, int max_vertices,
                            int max_triangles, int *inst_offsets, int *inst_mesh, int *inst_label, double *inst_pose,
                            int *inst_vert_base, int *inst_tri_base, long long *occ_class, float *occ_centre,
                            cloudaae_stream_t stream);

/* ---- object symmetries ("Object symmetries", has the definition) ---- */

/* The directed Hausdorff distance of m query points, moved by each of c rigid transforms, from n target points: queries
 * [m] and targets [n] are float points q_stride / t_stride floats apart (>= 3; the first three are read and widened to
 * double exactly), transforms [c,4,4] double row-major, top three rows read, applied as T x = ((A00 x + A01 y) + A02 z)
 * + A03 row by row.  All device memory.  In double, no fma: H2_c = max_i min_j ((dx dx + dy dy) + dz dz) with d = T_c x_i
 * - y_j; out [c] double = sqrt(H2_c) (correctly rounded) where H2_c <= limit2, else +inf.  limit2 >= 0, +inf allowed.
 * Minima and maxima are exact (the maxima as integer comparisons on the bit patterns), so the result does not depend on
 * the order of execution or the run.  A workgroup that finds its candidates' published maxima above limit2 already stops:
 * their result is +inf either way.  A memset and two launches.  workspace:
 * cloudaae_transform_hausdorff_workspace_bytes(c) bytes (-1 outside the limit on c), need not be initialised.
 * Limits: 1 <= c <= 2^20; 1 <= m, n <= 2^24; ceil(c / 4) * ceil(m / 128) < 2^31.  Outside them, with a stride below 3, a
 * limit2 that is negative or not a number, or a null pointer, the call returns an error and launches nothing. */
long long cloudaae_transform_hausdorff_workspace_bytes(int c);
int cloudaae_transform_hausdorff(int c, int m, const float *queries, int q_stride, int n, const float *targets, int t_stride,
                                 const double *transforms, double limit2, double *out, void *workspace,
                                 cloudaae_stream_t stream);

/* ---- equivalent poses ("Equivalent poses", has the definition) ---- */

/* The symmetry table of num_class classes, all device memory:
 *   sym_index  [num_class,3] int     kind, first, count of class i
 *   sym_centre [num_class,3] double  the symmetry centre c in the object frame (read for kinds with members)
 *   sym_axis   [num_class,3] double  the unit axis a (read for CLOUDAAE_SYMMETRY_AXIAL)
 *   sym_rot    [num_rot,9]   double  rotations, row-major 3x3; may be NULL when num_rot = 0
 * CLOUDAAE_SYMMETRY_NONE: no members (an object without symmetry; also what a spherical one is given: every rotation
 * is equivalent there and no label is nearer than another in a useful sense).  CLOUDAAE_SYMMETRY_FINITE: the count
 * rotations G_j = sym_rot[first + j], 1 <= count <= CLOUDAAE_SYMMETRY_MAX_MEMBERS, the identity first.
 * CLOUDAAE_SYMMETRY_AXIAL: every rotation about a, and with count = 1 also F = sym_rot[first], a half-turn about a
 * line perpendicular to a, times those; count is 0 or 1.  The index lives on the device, so the host cannot read it:
 * an entry with another kind, or whose first / count leave [0, num_rot] or the limits above, is treated as
 * CLOUDAAE_SYMMETRY_NONE by the kernel and never followed; so is a class_id outside [0, num_class). */
#define CLOUDAAE_SYMMETRY_NONE 0
#define CLOUDAAE_SYMMETRY_FINITE 1
#define CLOUDAAE_SYMMETRY_AXIAL 2
#define CLOUDAAE_SYMMETRY_MAX_MEMBERS 64

/* Of the poses T_label o [S | c - S c], S in the class's symmetry set, the one whose rotation is nearest the predicted
 * one.  rot_pred [b,3] axis-angle, float (rot_pred_is_f64 = 0) or double (1), widened exactly; rot_label [b,3] double,
 * trans_label [b,3] float, class_id [b] long long; the table as above.  In double, no fma, products and sums in the
 * written order; exp is the exponential map of cloudaae_exponential_map (the loss's op sequence).
 *   Rp = exp(rot_pred), Rl = exp(rot_label), M = Rp^T Rl: M[i][k] = (Rp[0][i] Rl[0][k] + Rp[1][i] Rl[1][k]) + Rp[2][i] Rl[2][k],
 *   so that tr(M S) is the trace the loss sees for the label Rl S.  tr X = (X00 + X11) + X22; a matrix product X Y has
 *   (X Y)[i][k] = (X[i][0] Y[0][k] + X[i][1] Y[1][k]) + X[i][2] Y[2][k].
 *   none:   S* = I, member = 0, phi = 0, s* = tr M; rot_equiv and trans_equiv are the labels, copied bit for bit.
 *   finite: s_j = (t_0 + t_1) + t_2 with t_i = (M[i][0] G_j[0][i] + M[i][1] G_j[1][i]) + M[i][2] G_j[2][i]; member = the
 *           smallest j with the largest s_j, S* = G_member, phi = 0.
 *   axial:  for the cosets E_0 = I and, with count = 1, E_1 = F:  N = M E_e (N = M itself for e = 0),
 *           u_i = (N[i][0] a0 + N[i][1] a1) + N[i][2] a2, alpha = (a0 u0 + a1 u1) + a2 u2, tau = tr N,
 *           beta = (a0 (N12 - N21) + a1 (N20 - N02)) + a2 (N01 - N10), d = tau - alpha,
 *           s_e = alpha + sqrt(d d + beta beta)  (the maximum of tr(N R_a(phi)) over phi),
 *           phi_e = atan2(beta, d), or 0 when d = beta = 0;
 *           member = the smallest e with the largest s_e, phi = phi_member, S* = E_member R_a(phi) (R_a itself for member 0)
 *           with R_a(phi)[i][k] = (delta_ik + sin(phi) K[i][k]) + (1 - cos(phi)) (K K)[i][k], K = [a]x.
 *   Where S* is the identity matrix exactly (member 0 of a finite set, or no turn about the axis) rot_equiv and trans_equiv
 *   are again the labels, copied bit for bit.  Otherwise
 *   rot_equiv [b,3] double = the log map of Rl S* as "Pose refinement" defines it for rot_out (theta = atan2(|v|, tr - 1),
 *           the axis from the symmetric part when cos < -0.5);
 *   trans_equiv [b,3] float = float(double(trans_label) + Rl w), w_i = c_i - (S* c)_i, (X v)_i = (X[i][0] v0 + X[i][1] v1)
 *           + X[i][2] v2: the translation of T_label o [S* | c - S* c], the convention of cloudaae_pose_max_dist's G (S x);
 *   member [b] int, phi [b] double, angle [b] double = acos(clamp((s* - 1) / 2, -0.9999999, 0.9999999)), the loss's clamp.
 * One wave per sample, one launch, no workspace, no atomics: bit-reproducible and independent of b.
 * Errors (nothing is launched): b outside [1, 2^24]; rot_pred_is_f64 not 0 or 1; num_class < 1; num_rot outside
 * [0, 2^24]; a null pointer (sym_rot may be NULL only with num_rot = 0). */
int cloudaae_nearest_equivalent_pose(int b, const void *rot_pred, int rot_pred_is_f64, const double *rot_label,
                                     const float *trans_label, const long long *class_id, int num_class,
                                     const int *sym_index, const double *sym_centre, const double *sym_axis, int num_rot,
                                     const double *sym_rot, double *rot_equiv, float *trans_equiv, int *member, double *phi,
                                     double *angle, cloudaae_stream_t stream);

/* ---- pose verification ("Pose verification", has the definition) ---- */

/* p hypotheses per sample from a base pose and the class's transform set.  base [b,16] double (row-major 4x4, top three
 * rows read), class_id [b] long long; the table: hyp_index [nclass+1] int, offsets into hyp [n_total,16] double (row-major
 * 4x4, top three rows read) -- class c owns members hyp_index[c] .. hyp_index[c+1] - 1, the first of which is the identity
 * by the caller's contract.  All device memory.  Hypothesis j of sample i is base_i H_{c,j}, in double, no fma:
 *   C[r][k] = (A[r][0] H[0][k] + A[r][1] H[1][k]) + A[r][2] H[2][k]                 k = 0, 1, 2
 *   C[r][3] = ((A[r][0] H[0][3] + A[r][1] H[1][3]) + A[r][2] H[2][3]) + A[r][3]
 * with A = base_i.  j >= the class's count repeats member 0 and sets valid to 0; a class_id outside [0, nclass), or an
 * entry whose offsets leave [0, n_total] or run backwards, is an empty set: H = I for every j, valid 0, and hyp is not read.
 * Outputs: pose [b,p,16] double (bottom row 0 0 0 1), rot_axag [b,p,3] double = the log map of C's rotation as "Pose
 * refinement" defines it for rot_out (angle in [0, pi]), trans [b,p,3] float = float(C[r][3]), valid [b,p] int.
 * One launch, one lane per hypothesis, no atomics: bit-reproducible and independent of b.
 * Limits: b, p >= 1; b * p <= 2^28; nclass >= 1; 0 <= n_total <= 2^24; outside them, or with a null pointer (hyp may be
 * NULL only with n_total = 0), the call returns an error and launches nothing. */
int cloudaae_pose_compose(int b, const double *base, const long long *class_id, int nclass, const int *hyp_index, int n_total,
                          const double *hyp, int p, double *pose, double *rot_axag, float *trans, int *valid,
                          cloudaae_stream_t stream);

/* How each of p rendered hypotheses of b samples agrees with the depth the camera saw.  depth_test [f,h,w] uint16;
 * label [f,h,w] uint8 or NULL; frame_of [b] int: the test frame of each sample; want [b] int: the label value of the
 * sample's object (may be NULL with label NULL); depth_hyp [b,p,h,w] uint16: the object's mesh alone, rendered with that
 * frame's intrinsics (so the same factor_depth); tau [b] int, in depth units.  All device memory.
 * Integer arithmetic on the uint16 values widened to int, no floating point.  Per pixel, t = test depth, d = hypothesis
 * depth, seg = (label != NULL and label == want and t != 0):
 *   rendered   d != 0
 *   consistent d != 0 and t != 0 and |d - t| <= tau
 *   in_front   d != 0 and t != 0 and t - d > tau     (the camera saw through the hypothesis)
 *   behind     d != 0 and t != 0 and d - t > tau     (hidden by something nearer)
 *   unknown    d != 0 and t == 0
 *   explained  seg and consistent
 * Outputs (zeroed by the call): counts [b,p,6] int in that order; seg_total [b] int = #seg; abs_sum [b,p] long long = the
 * sum of |d - t| over the consistent pixels.  Three memsets and one launch; integer atomics only, so the results do not
 * depend on the order of execution, the batch or the run.  A frame_of entry outside [0, f) leaves that sample's counts 0
 * and causes no access.  Limits: f, h, w, b, p >= 1; h * w <= 2^24; b * p * h * w <= 2^28; outside them, or with a null
 * pointer other than label (and want with it), the call returns an error and launches nothing. */
int cloudaae_depth_fit_counts(int f, int h, int w, const uint16_t *depth_test, const uint8_t *label, int b, int p,
                              const int *frame_of, const int *want, const uint16_t *depth_hyp, const int *tau, int *counts,
                              int *seg_total, long long *abs_sum, cloudaae_stream_t stream);

/* The winner among the p hypotheses of each sample.  counts [b,p,6], seg_total [b] as cloudaae_depth_fit_counts writes
 * them, valid [b,p] int, pose [b,p,16] double.  mode 0 (the segment rule): num = explained, den = seg_total + in_front;
 * mode 1 (the silhouette rule, for callers without a label): num = consistent, den = (consistent + in_front) + behind.
 * A hypothesis with den <= 0, num < 0 or valid = 0 has num = 0, den = 1.  Hypothesis j beats k when num_j den_k >
 * num_k den_j in 64-bit integers (exact: num <= 2^24, den < 2^26); best [b] int is the lowest index that no other beats.
 * score [b,p] double = (double)num / (double)den; pose_best [b,16] double = pose[best], copied bit for bit; margin [b]
 * double = score[best] - the largest score among the others, 0 for p = 1.  One launch, one lane per sample, no atomics.
 * Limits: b, p >= 1; b * p <= 2^28; mode 0 or 1; outside them, or with a null pointer, the call returns an error and
 * launches nothing. */
int cloudaae_select_pose(int b, int p, const int *counts, const int *seg_total, const int *valid, const double *pose,
                         int mode, int *best, double *score, double *pose_best, double *margin, cloudaae_stream_t stream);

/* ---- pose proposals by point-pair-feature voting ("Pose proposals", has the definition) ---- */

/* Shared by the three calls below.  Arithmetic: double on the float points widened exactly, + - * / sqrt only, no fma,
 * products and sums in the written order.  No angle is formed on the device: cos_edges [n_angle-1] double holds
 * cos(k pi / n_angle), k = 1 .. n_angle-1, and bin(c) = #{k : c <= cos_edges[k-1]}; alpha_edges [n_alpha/2 - 1] double holds
 * cos(k pi / (n_alpha/2)) likewise, and alpha_cs [n_alpha,2] double the cosine and sine of the bin centres
 * -pi + (j + 1/2) 2 pi / n_alpha.  The host makes the tables; whoever reads the same tables gets the same integers.
 *   key(p1, n1, p2, n2): d = p2 - p1, len = sqrt((dx dx + dy dy) + dz dz); none when !(len > 0); t = len / dist_step, none
 *     unless 0 <= t < n_dist; q_d = (int)t; c1 = ((n1.x dx + n1.y dy) + n1.z dz) / len, c2 the same with n2,
 *     c3 = (n1.x n2.x + n1.y n2.y) + n1.z n2.z; key = ((q_d n_angle + bin(c1)) n_angle + bin(c2)) n_angle + bin(c3).
 *     Normals are taken as unit vectors and are not normalised again.
 *   Q(n), the rotation taking n onto +x: row 0 = n; with h = 1 + |n.x| and a = (n.y n.z) / h,
 *     n.x >= 0: row 1 = (-n.y, 1 - (n.y n.y) / h, -a),    row 2 = (-n.z, -a, 1 - (n.z n.z) / h);
 *     n.x <  0: row 1 = (-n.y, -(1 - (n.y n.y) / h), a),  row 2 = ( n.z, -a, 1 - (n.z n.z) / h)   (Q(-n), then a half turn about z).
 *   direction(n1, d): y = (Q10 dx + Q11 dy) + Q12 dz, z = (Q20 dx + Q21 dy) + Q22 dz with Q = Q(n1), r = sqrt(y y + z z); none
 *     when !(r > 0); else (y / r, z / r). */

/* The pair table of s packed point sets: offsets [s+1] int into xyz [m_total,3] float and normals [m_total,3] double;
 * pair_offsets [s+1] long long, pair_offsets[i+1] - pair_offsets[i] = M_i^2; dist_step [s] double.  All device memory.  For
 * the ordered pair (r, i) of set j, entry e = pair_offsets[j] + r M_j + i gets key [e] int = key(p_r, n_r, p_i, n_i), or -1
 * for i = r, a pair without a key or without a direction; ref [e] int = r; dir [e,2] float = (float) direction(n_r, p_i - p_r),
 * zeros with key -1.  A set whose offsets leave [0, m_total] or whose pairs leave [0, n_pairs) is not written.  One
 * launch, one wave per point.  Limits: 1 <= s <= 2^20; 1 <= m_total <= 2^24; 1 <= n_pairs <= 2^28; n_dist >= 1;
 * 1 <= n_angle <= 64; n_dist n_angle^3 <= 2^24; outside them, or with a null pointer, an error and no launch. */
int cloudaae_ppf_model_pairs(int s, const int *offsets, const long long *pair_offsets, int m_total, long long n_pairs,
                             const float *xyz, const double *normals, const double *dist_step, int n_dist, int n_angle,
                             const double *cos_edges, int *key, int *ref, float *dir, cloudaae_stream_t stream);

/* Voting.  scene [b,n,3] float, scene_normals [b,n,3] double, mask [b,n] uint8 (non-zero: usable), class_id [b] long long.
 * The models: offsets [nclass+1] int into model_xyz [m_total,3] float / model_normals [m_total,3] double, dist_step [nclass]
 * double, bucket_start [nclass, n_key+1] int (n_key = n_dist n_angle^3): the entries of key k of class c are
 * bucket_start[c][k] .. bucket_start[c][k+1] - 1 of entry_ref [n_entries] int (the model point r, local to its set) and
 * entry_dir [n_entries,2] float.  All device memory.
 * R = ceil(n / ref_step) reference slots per sample; slot j's reference point is usable point number j ref_step of the
 * sample in index order (an empty slot when there are fewer).  One workgroup per (sample, slot) keeps m_max n_alpha
 * int counters in LDS (zeroed).  For every other usable point i with k = key(p_ref, n_ref, p_i, n_i) and u = direction(n_ref,
 * p_i - p_ref), and every entry e of the bucket clamped to [0, n_entries) with 0 <= entry_ref[e] < M_c:  w = entry_dir[e],
 * ca = u.y w.y + u.z w.z, sa = u.z w.y - u.y w.z (alpha = alpha_scene - alpha_model), q = #{k : ca <= alpha_edges[k-1]},
 * bin = sa >= 0 ? n_alpha/2 + q : n_alpha/2 - 1 - q; counter [entry_ref[e] n_alpha + bin] += 1.
 * A class_id outside [0, nclass), a model with offsets that leave [0, m_total] or M_c outside [1, m_max], or an empty slot
 * reads no table and leaves all counters 0.
 * Peak k = 0 .. peaks-1 is the k-th cell by (votes descending, cell index ascending): votes [b,R,peaks] int, model_index
 * = cell / n_alpha, bin = cell % n_alpha (both -1 where votes = 0) and pose [b,R,peaks,16] double = T_s^-1 Rx T_m (the identity
 * where votes = 0) with (ca, sa) = alpha_cs[bin], Qm = Q(n_model), Qs = Q(n_ref):
 *   A[0][k] = Qm[0][k], A[1][k] = ca Qm[1][k] - sa Qm[2][k], A[2][k] = sa Qm[1][k] + ca Qm[2][k];
 *   R[i][k] = (Qs[0][i] A[0][k] + Qs[1][i] A[1][k]) + Qs[2][i] A[2][k];  t[i] = p_ref[i] - ((R[i][0] pm.x + R[i][1] pm.y) + R[i][2] pm.z).
 * acc: NULL, or [b,R,m_max,n_alpha] int that receives every counter.  Integer LDS atomics only: the result depends on no
 * order, batch or run.  Limits: b >= 1; 2 <= n <= 2^20; 1 <= ref_step <= n; b R <= 2^24; 1 <= peaks <= 4 <= m_max n_alpha;
 * n_alpha even in [2, 128]; 4 m_max n_alpha <= 158 KiB; 0 <= n_entries <= 2^28; the limits of cloudaae_ppf_model_pairs on
 * n_dist, n_angle and m_total; 1 <= m_max <= m_total.  Outside them, or with a null pointer (acc aside; the entries may be
 * NULL with n_entries = 0), an error and no launch. */
int cloudaae_ppf_vote(int b, int n, const float *scene, const double *scene_normals, const uint8_t *mask,
                      const long long *class_id, int ref_step, int peaks, int nclass, const int *offsets, int m_total, int m_max,
                      const float *model_xyz, const double *model_normals, const double *dist_step, int n_dist, int n_angle,
                      int n_alpha, const double *cos_edges, const double *alpha_edges, const double *alpha_cs,
                      const int *bucket_start, long long n_entries, const int *entry_ref, const float *entry_dir, int *votes,
                      int *model_index, int *bin, double *pose, int *acc, cloudaae_stream_t stream);

/* Greedy clustering of c candidates per sample: votes [b,c] int, pose [b,c,16] double, class_id [b] long long,
 * trans_thresh2 [nclass] double (the squared translation threshold of each class), rot_bound = 1 + 2 cos(rot_thresh).
 * Candidates with votes > 0 are visited by (votes descending, index ascending).  A candidate b joins the first cluster,
 * in founding order, whose representative a has (dx dx + dy dy) + dz dz <= trans_thresh2 (d = t_a - t_b) and
 * (r_0 + r_1) + r_2 >= rot_bound, r_i = (Ra[i][0] Rb[i][0] + Ra[i][1] Rb[i][1]) + Ra[i][2] Rb[i][2]; otherwise it founds one
 * and is its representative.  A cluster's score is the sum of its members' votes.  A class_id outside [0, nclass) gives no
 * cluster.  Slot t = 0 .. top-1 is the t-th cluster by (score descending, founding order ascending): pose_out [b,top,16] =
 * its representative's pose bit for bit, rot_axag [b,top,3] double = the log map of "Pose refinement", trans [b,top,3]
 * float, score [b,top] int, valid [b,top] int = 1; past the clusters the identity, zeros and valid 0.  One launch, one wave
 * per sample, no atomics.  Limits: 1 <= b <= 2^24; 1 <= c <= 4096; 1 <= top <= 64; nclass >= 1; rot_bound a number.
 * Outside them, or with a null pointer, an error and no launch. */
int cloudaae_ppf_cluster(int b, int c, const int *votes, const double *pose, const long long *class_id, int nclass,
                         const double *trans_thresh2, double rot_bound, int top, double *pose_out, double *rot_axag, float *trans,
                         int *score, int *valid, cloudaae_stream_t stream);

/* ---- object candidates from unlabelled depth frames ("Depth components", has the definition) ---- */

/* Shared by the calls below.  depth [f,h,w] uint16, intrinsics [f,5] float (fx, fy, cx, cy, factor_depth); pixel (u, v) has
 * index p = v w + u within its frame and is valid when its depth is not 0.  Points are back-projected in fp32 as
 * cloudaae_frame_segments does, then widened; everything after is double, + - * in the written order, no fma.  All
 * memory is device memory.  Limits of every call: f >= 0; h, w >= 1; h w <= 2^24; f h w <= 2^28; outside them, or with a
 * null pointer, an error and no launch.  f = 0 is not an error: nothing is launched and nothing written. */

/* The dominant plane of each frame.  Hypothesis hy of frame fr: r = philox4x32(seed, ((first_frame + fr) << 20) | hy, stream
 * 25); its pixels p_k = (r[k] (h w)) >> 32, k = 0, 1, 2; void when one of them is invalid; n = (P1 - P0) x (P2 - P0), each
 * component a b - c d; q = (nx nx + ny ny) + nz nz, void unless q > 0; d = -((nx P0x + ny P0y) + nz P0z); n and d change sign
 * when d < 0.  The tested pixels are the valid ones with u and v multiples of stride; P is an inlier when s s <= (tol tol) q,
 * s = ((nx Px + ny Py) + nz Pz) + d.  count [f,n_hyp] int (0 for a void hypothesis) and tested [f] int are zeroed by the
 * call.  The winner is the largest count, ties to the lowest hy; the frame has a plane when count >= 3 and count 100 >=
 * min_plane_percent tested: plane [f,4] double = (n, d) of the winner, un-normalised, and plane_hyp [f] int = hy; otherwise
 * zeros and -1.  Two memsets and two launches; integer atomics only.  Limits: 1 <= n_hyp <= 4096; stride >= 1;
 * 0 <= first_frame <= 2^40; 0 <= min_plane_percent <= 100; tol >= 0. */
int cloudaae_depth_plane(int f, int h, int w, const uint16_t *depth, const float *intrinsics, unsigned long long seed,
                         long long first_frame, int n_hyp, int stride, double tol, int min_plane_percent, int *count,
                         int *tested, double *plane, int *plane_hyp, cloudaae_stream_t stream);

/* fg [f,h,w] uint8 (1 or 0).  A frame with plane_hyp >= 0: valid and s > 0 and s s > (tol tol) q and s s <= (max_height
 * max_height) q, with q formed again from plane [f,4]; a frame with plane_hyp < 0: valid.  One launch.  tol, max_height >= 0. */
int cloudaae_depth_foreground(int f, int h, int w, const uint16_t *depth, const float *intrinsics, const double *plane,
                              const int *plane_hyp, double tol, double max_height, uint8_t *fg, cloudaae_stream_t stream);

/* Connected components.  Two 4-adjacent pixels are joined when both have fg != 0 and their depths, widened to int, differ by
 * at most jump_units [f] int (a negative entry joins nothing).  root [f,h,w] int = the smallest pixel index of the pixel's
 * component, -1 where fg = 0: a pure function of the input.  status [f] int is zeroed by the call; a bit is set when a
 * bounded walk ran into its bound (1: inside a tile, 2: across tile borders, 4: the final walk), which no input should
 * cause -- the roots of that frame are then not to be trusted.  One memset and three launches (32 x 32 tiles in LDS, the
 * pixel pairs across tile borders, the final roots); no workgroup waits for another. */
long long cloudaae_depth_components_workspace_bytes(int f, int h, int w);
int cloudaae_depth_components(int f, int h, int w, const uint16_t *depth, const uint8_t *fg, const int *jump_units, int *root,
                              int *status, void *workspace, long long workspace_bytes, cloudaae_stream_t stream);

/* Concave creases of the foreground ("Creases", has the definition): the cut that separates touching objects
 * before cloudaae_depth_components labels them.  fg [f,h,w] uint8 as cloudaae_depth_foreground writes it (any non-zero
 * value counts); step s, smooth r, cos2 = cos(angle)^2.
 * Stage 1, integers.  For a foreground pixel c of a frame with jump_units >= 0 the members of its box are the pixels q of the
 * frame with |u_q - u_c| <= r, |v_q - v_c| <= r, fg != 0 and |d_q - d_c| <= jump_units (depths widened to int; c itself is
 * one): S their depths' sum, n their number, smooth_map = (S << 8) | n; elsewhere smooth_map = 0.  The workspace's first
 * f h w words ARE smooth_map [f,h,w] uint32, written by every call and readable afterwards.
 * The smoothed point of a pixel, double, un-fused: z = (double)S / ((double)n * (double)factor_depth), x = (((double)u -
 * (double)cx) * z) / (double)fx, y likewise.
 * Stage 2.  Direction bit b = 0 .. 3 is (du, dv) = (1,0), (0,1), (1,1), (1,-1); A = (u - s du, v - s dv), B = (u + s du,
 * v + s dv).  The direction is tested at a foreground pixel C when A and B are pixels of the frame, both foreground, and
 * |d_A - d_C| <= s jump_units and |d_B - d_C| <= s jump_units on the raw depths (64-bit product).  With e1 = P_A - P_C,
 * e2 = P_B - P_C on smoothed points: g = (e1x e2x + e1y e2y) + e1z e2z; m = e1 + e2; cc = (mx Cx + my Cy) + mz Cz; q1, q2 the
 * squared lengths formed like g.  The bit is set when the direction is tested, cc < 0 and (g >= 0 or g g < cos2 (q1 q2)).
 * Outputs, all written: crease, tested [f,h,w] uint8 (the four bits), fg_cut [f,h,w] uint8 = 1 where fg != 0 and crease = 0,
 * n_crease [f] int = the pixels with crease != 0.  One memset and two launches, both 32 x 32 tiles staged in LDS with a halo
 * of r and of s pixels; one integer atomic per workgroup; no workgroup waits for another.  Limits: 1 <= step <= 8;
 * 0 <= smooth <= 7 (so that S < 2^24 and n < 2^8); cos2 a number in [0, 1]. */
long long cloudaae_depth_creases_workspace_bytes(int f, int h, int w);
int cloudaae_depth_creases(int f, int h, int w, const uint16_t *depth, const uint8_t *fg, const float *intrinsics,
                           const int *jump_units, int step, int smooth, double cos2, uint8_t *crease, uint8_t *tested,
                           uint8_t *fg_cut, int *n_crease, void *workspace, long long workspace_bytes,
                           cloudaae_stream_t stream);

/* The component table of root [f,h,w] int as cloudaae_depth_components writes it (an entry outside [0, h w) counts as
 * background).  The candidates of a frame are the components of at least min_pixels pixels, ordered by (size descending,
 * root ascending); the first K = min(candidates, max_components) are kept.  label [f,h,w] uint8 = k + 1 on the pixels of
 * component k, else 0; n_components [f] int = K; n_candidates [f] int = the candidates before the cap; comp_root, comp_size
 * [f,max_components] int and comp_box [f,max_components,4] int = (u_min, v_min, u_max, v_max), -1 past K.  One memset and
 * four launches; integer atomics only.  Limits: min_pixels >= 1; 1 <= max_components <= 254. */
long long cloudaae_component_labels_workspace_bytes(int f, int h, int w);
int cloudaae_component_labels(int f, int h, int w, const int *root, int min_pixels, int max_components, uint8_t *label,
                              int *n_components, int *n_candidates, int *comp_root, int *comp_size, int *comp_box,
                              void *workspace, long long workspace_bytes, cloudaae_stream_t stream);

/* ---- detections: which component is which object ("Detections", has the definition) ---- */

/* cloudaae_depth_fit_counts over a window of wh x ww pixels per sample.  depth_test [f,h,w] uint16; label [f,h,w] uint8 or
 * NULL; frame_of, want, tau [b] int as there; origin [b,2] int = (u0, v0), any values, negative or past the frame included;
 * depth_hyp [b,p,wh,ww] uint16: the hypothesis rendered into the window (intrinsics with cx - u0, cy - v0).  All device
 * memory.  Window pixel (x, y), 0 <= x < ww, 0 <= y < wh, is frame pixel (u0 + x, v0 + y); where that lies outside the frame
 * t = 0 and the pixel is not in the segment, and nothing is read.  Per window pixel t, d, seg and the six predicates are
 * those of cloudaae_depth_fit_counts; hypothesis pixels outside the window do not exist for this call.  Outputs (zeroed
 * by the call): counts [b,p,6] int, seg_total [b] int = #seg inside the window, abs_sum [b,p] long long.  With origin (0, 0),
 * wh = h and ww = w every output equals cloudaae_depth_fit_counts's.  Three memsets and one launch; integer atomics only,
 * so the results do not depend on the order of execution, the batch or the run.  A frame_of entry outside [0, f) leaves
 * that sample's counts 0 and causes no access.  Any ww >= 1 is taken (a lane's eight pixels may straddle rows); 16-byte
 * loads are used only where an address allows it.  Limits: f, h, w, b, p, wh, ww >= 1; h * w <= 2^24; wh * ww <= 2^24;
 * b * p * wh * ww <= 2^28; outside them, or with a null pointer other than label (and want with it), the call returns an
 * error and launches nothing. */
int cloudaae_depth_fit_counts_window(int f, int h, int w, const uint16_t *depth_test, const uint8_t *label, int b, int p,
                                     const int *frame_of, const int *want, const int *origin, int wh, int ww,
                                     const uint16_t *depth_hyp, const int *tau, int *counts, int *seg_total, long long *abs_sum,
                                     cloudaae_stream_t stream);

/* The decision over the (component, class) pairs of each frame.  counts [f,k,c,p,6] and seg_total [f,k,c] int as
 * cloudaae_depth_fit_counts_window writes them for sample (fr k + kk) c + cc; valid [f,k,c,p] int; pose [f,k,c,p,16] double;
 * n_components [f] int (clamped into [0, k]); mode 0 or 1: the two rules of cloudaae_select_pose; the threshold min_num /
 * min_den; max_per_class.  All device memory.
 * Step 1.  The fraction of a hypothesis is cloudaae_select_pose's (num, den), and 0 / 1 when den <= 0, num < 0, valid = 0 or
 * kk >= n_components.  Hypothesis j beats i when num_j den_i > num_i den_j in 64-bit integers (exact for counts that
 * cloudaae_depth_fit_counts_window wrote: num <= 2^24, den < 2^26); pair_hyp [f,k,c] int is the lowest index that no other
 * beats, pair_num, pair_den [f,k,c] int its fraction and pair_score [f,k,c] double = (double)num / (double)den.
 * Step 2, at most n_components rounds.  A pair is eligible when its component is unassigned, its class has been assigned
 * fewer than max_per_class times, num > 0 and num min_den >= min_num den.  The eligible pair with the largest fraction,
 * compared as above, ties to the lowest kk and then the lowest cc, is assigned in round r = 0, 1, ...; the rounds end
 * when nothing is eligible.
 * Outputs per (fr, kk), all written: det_class int (-1: none), det_hyp int = pair_hyp of the assigned pair (-1), det_num,
 * det_den int (0, 1), det_score double = (double)det_num / (double)det_den, det_rank int = r (-1), det_pose [16] double =
 * pose of the chosen hypothesis bit for bit (zeros); alt_class, alt_num, alt_den int: the pair of the same component with
 * the largest fraction among the classes other than det_class (all classes when there is none), availability and the
 * threshold ignored, ties to the lowest cc; -1, 0, 1 when c = 1 leaves no other class.  n_det [f] int = the assignments.
 * One launch, one workgroup per frame, no atomics; no workgroup waits for another and every loop is bounded.
 * Limits: f >= 1; 1 <= k <= 254; 1 <= c <= 256; 1 <= p <= 64; f k c p <= 2^28; 0 <= min_num <= min_den; 1 <= min_den <=
 * 2^20; max_per_class >= 1; outside them, or with a null pointer, the call returns an error and launches nothing. */
int cloudaae_detect_assign(int f, int k, int c, int p, const int *counts, const int *seg_total, const int *valid,
                           const double *pose, const int *n_components, int mode, int min_num, int min_den, int max_per_class,
                           int *pair_hyp, int *pair_num, int *pair_den, double *pair_score, int *det_class, int *det_hyp,
                           int *det_num, int *det_den, double *det_score, int *det_rank, double *det_pose, int *alt_class,
                           int *alt_num, int *alt_den, int *n_det, cloudaae_stream_t stream);

/* ---- tracking: depth-image alignment of known objects across frames ("Tracking", has the definition) ---- */

/* One Gauss-Newton step of dense point-to-plane alignment for b tracks.  depth_test [f,h,w] uint16; frame_of [b] int; origin
 * [b,2] int = (u0, v0) and one wh, ww per call: window pixel (x, y) is frame pixel (u0 + x, v0 + y), as for
 * cloudaae_depth_fit_counts_window; depth_hyp [b,wh,ww] uint16: the object alone, rendered at pose_in into its window;
 * intr_win [b,5] float: the window's row (fx, fy, cx - u0, cy - v0, factor_depth); gate, jump [b] int in depth units; cos_min;
 * pose_in [b,16] double.  All device memory.  Arithmetic: double on exactly widened integers and floats, un-fused, in the
 * written order.
 * P(x, y, z) = (((x - cxw) dm) / fx, ((y - cyw) dm) / fy, dm), dm = z / factor_depth, (x, y) WINDOW coordinates in either
 * image.  The normal of an image at a pixel s of depth z_s: a neighbour is valid when it lies inside the image (the window
 * for depth_hyp, the frame for depth_test), has depth != 0 and |z_nb - z_s| <= jump; along x: gx = P(x+1) - P(x-1) when both
 * are valid, P(x+1) - P(s) or P(s) - P(x-1) with the one valid neighbour, else the axis has no slope; gy likewise; n = gx x gy,
 * each component (p q) - (r s); nn = (nx nx + ny ny) + nz nz; the pixel is flat when an axis has no slope or nn is 0 or not
 * finite; the unit normal is each component divided by sqrt(nn), its sign as it comes.
 * A window pixel with d = depth_hyp and t = the frame pixel's depth (0 outside the frame) is a pair when d != 0, t != 0,
 * |d - t| <= gate, the hypothesis normal n at (x, y) is not flat and, when cos_min > 0, the observed normal m at the frame
 * pixel is not flat and |(nx mx + ny my) + nz mz| >= cos_min; cos_min <= 0 reads no observed neighbour.
 * Per pair p = P(x, y, d), q = P(x, y, t), e = p - q, r = (ex nx + ey ny) + ez nz, a = p x n = (py nz - pz ny, pz nx - px nz,
 * px ny - py nx), J = (a, n); A = sum J J^T, b = sum J r; A x = -b by LDL^T without pivoting and U from x exactly as in
 * cloudaae_icp_point_to_plane.
 * Outputs, all written: n_pairs [b] int; sums [b,28] double = sum r r, A's upper triangle by rows, b; x [b,6] double (zeros
 * unless status is 0); status [b] int: 0 updated, 1 fewer than six pairs, 2 a pivot that is not a finite number > 0, 3 a
 * solution that is not finite, 4 frame_of outside [0, f) (nothing of that sample is read; n_pairs and sums are 0);
 * pose_out [b,16] double = U pose_in with the products formed as cloudaae_pose_compose forms them and the last row 0 0 0 1;
 * for every status but 0 pose_in bit for bit.
 * Two launches: a workgroup of 256 lanes adds a run of 2048 window pixels, eight consecutive per lane in pixel order, the wave
 * by a butterfly, the four waves in order, and stores 28 partial sums and a count to the workspace; one wave per sample adds
 * the runs in run order and solves.  No floating-point atomics and no workgroup waits for another: the same bits run to run
 * and whatever else is in the batch.  workspace: cloudaae_depth_align_step_workspace_bytes(b, wh, ww) bytes, 8-byte aligned
 * (0: outside the limits).  Limits: f, h, w, b, wh, ww >= 1; h * w <= 2^24; wh * ww <= 2^24; b * wh * ww <= 2^28; outside
 * them, with a null pointer, a workspace too small or cos_min not a number the call returns an error and launches nothing. */
long long cloudaae_depth_align_step_workspace_bytes(int b, int wh, int ww);
int cloudaae_depth_align_step(int f, int h, int w, const uint16_t *depth_test, int b, const int *frame_of, const int *origin,
                              int wh, int ww, const uint16_t *depth_hyp, const float *intr_win, const int *gate,
                              const int *jump, double cos_min, const double *pose_in, int *n_pairs, double *sums, double *x,
                              int *status, double *pose_out, void *workspace, long long workspace_bytes,
                              cloudaae_stream_t stream);

/* ---- tracking: the occluding-contour term ("Contours", has the definition) ---- */

/* Shared by the three entries below: the arguments named as in cloudaae_depth_align_step mean the same; its limits and error
 * rules apply (an error launches nothing), and in addition 1 <= radius <= 32.  The edge mask of a pixel with depth z != 0 of
 * an image: bits 0..3 stand for the neighbours (x-1, y), (x+1, y), (x, y-1), (x, y+1); a bit is set when that neighbour lies
 * inside the image (the frame for depth_test, the window for depth_hyp) and has z_nb = 0 or z_nb - z > step, in integers; a
 * pixel with z = 0 has mask 0; an edge pixel is one with mask != 0. */

/* The nearest observed edge of every window pixel.  step [b] int, device memory, in depth units.  nearest [b,wh,ww] int: -1,
 * or (mask_obs << 16) | ((j + radius) << 8) | (i + radius) for the offset (i, j) smallest in (i i + j j, j, i) among those
 * with i i + j j <= radius^2 whose frame pixel (u0 + x + i, v0 + y + j) lies inside the frame and is an edge pixel of
 * depth_test.  A sample whose frame_of lies outside [0, f) reads nothing and is all -1.  One launch, one workgroup per tile of
 * 32 x 32 window pixels. */
int cloudaae_depth_edge_nearest(int f, int h, int w, const uint16_t *depth_test, int b, const int *frame_of, const int *origin,
                                int wh, int ww, const int *step, int radius, int *nearest, cloudaae_stream_t stream);

/* The sums of the contour rows.  A window pixel (x, y) with d = depth_hyp(x, y) is a pair when its mask in depth_hyp is not
 * 0, nearest(x, y) >= 0 with offset (i, j) and mask_obs, |d - t_c| <= gate for the frame's depth t_c at (u0 + x + i, v0 + y +
 * j), and the two masks are equal.  With p = P(x, y, d) and dm = p_z a pair gives the row r = ((-i) dm) / fx, g = (1, 0,
 * -(p_x / p_z)) and then the row r = ((-j) dm) / fy, g = (0, 1, -(p_y / p_z)); J = (p x g, g), the cross product formed as in
 * cloudaae_depth_align_step.  n_rows [b] int = 2 x pairs; sums [b,28] double in the layout of cloudaae_depth_align_step, the
 * rows taken in pixel order.  Two launches, runs of 2048 window pixels, as cloudaae_depth_align_step; the same bits run to run
 * and whatever else is in the batch.  workspace: cloudaae_depth_contour_sums_workspace_bytes(b, wh, ww) bytes, 8-byte aligned
 * (0: outside the limits). */
long long cloudaae_depth_contour_sums_workspace_bytes(int b, int wh, int ww);
int cloudaae_depth_contour_sums(int f, int h, int w, const uint16_t *depth_test, int b, const int *frame_of, const int *origin,
                                int wh, int ww, const uint16_t *depth_hyp, const float *intr_win, const int *gate,
                                const int *step, int radius, const int *nearest, int *n_rows, double *sums, void *workspace,
                                long long workspace_bytes, cloudaae_stream_t stream);

/* The combined step: total[k] = plane_sums[k] + weight * contour_sums[k] (one multiply, one add), k < 28.  status [b]: 4
 * where plane_status is 4; else 1 where n_pairs + n_rows < 6; else the LDL^T solve, x -> U and pose_out = U pose_in of
 * cloudaae_depth_align_step on the totals, with its statuses 0, 2 and 3.  x [b,6] is zeros and pose_out [b,16] is pose_in bit
 * for bit for every status but 0.  plane_sums, n_pairs and plane_status are the sums, n_pairs and status that
 * cloudaae_depth_align_step wrote.  1 <= b <= 2^28; weight must be a number.  One launch, one wave per sample. */
int cloudaae_depth_align_solve(int b, const double *plane_sums, const int *n_pairs, const int *plane_status,
                               const double *contour_sums, const int *n_rows, double weight, const double *pose_in, double *x,
                               int *status, double *pose_out, cloudaae_stream_t stream);

/* ---- fused models: a signed distance volume from posed depth frames, and its mesh ("Fused models") ---- */

/* Shared by the three entries below.  The volume has nx x ny x nz voxels of side `voxel` (metres, in the object's frame); the
 * centre of voxel (i, j, k) is (ox + (i + 0.5) voxel, oy + (j + 0.5) voxel, oz + (k + 0.5) voxel) and its linear index (k ny +
 * j) nx + i.  state [nz,ny,nx,4] int, device memory, 16-byte aligned: (acc, cnt, acc_deep, cnt_deep) per voxel; the caller
 * zeroes it before the first frame.  Limits: 2 <= nx, ny, nz <= 512, nx ny nz <= 2^27; the origin finite, the voxel finite and
 * positive.  Outside them, or with a null required pointer, a call returns an error and launches nothing. */

/* Adds f frames to the state.  depth [f,h,w] uint16; label [f,h,w] uint8 and want [f] int, both or neither (either null: every
 * pixel with depth != 0 is used; else a pixel of frame g is used when want[g] == 0 or label == want[g]); intr [f,5] float:
 * fx, fy, cx, cy, factor_depth; poses [f,16] double, row-major 4 x 4, model -> camera.  Per voxel centre (x, y, z) and frame,
 * in float64 on exactly widened values, un-fused: X = ((A0 x + A1 y) + A2 z) + A3, Y and Z alike; nothing unless Z > z_near;
 * u' = ((fx X) / Z + cx) + 0.5, v' alike; nothing unless 0 <= u' < w and 0 <= v' < h (a NaN fails); d = depth at (floor u',
 * floor v'); nothing when d = 0 or the pixel is not used; sdf = d / factor_depth - Z; q = (int) rint(((sdf < front ? sdf :
 * front) / front) * 4096); sdf >= -behind: acc += q, cnt += 1; else sdf >= -front: acc_deep += q, cnt_deep += 1.  The sums are
 * integers: any split of the frames over calls and any order of the frames gives the same state bit for bit; they wrap
 * silently beyond 2^19 votes per voxel over all calls.  Limits: 1 <= f <= 2^19, h, w >= 1, h w <= 2^24; front, behind and
 * z_near finite, front > behind > 0, z_near > 0.  One launch, a lane per voxel, no atomics. */
int cloudaae_tsdf_integrate(int nx, int ny, int nz, double ox, double oy, double oz, double voxel, int *state, int f, int h,
                            int w, const uint16_t *depth, const uint8_t *label, const int *want, const float *intr,
                            const double *poses, double front, double behind, double z_near, cloudaae_stream_t stream);

/* Marching tetrahedra on the voxel centres.  A voxel's value is acc / cnt when cnt >= min_count, else acc_deep / cnt_deep when
 * cnt_deep >= 1, else unknown; it is inside when the value is < 0.  Cell (i, j, k), 0 <= i < nx - 1 (j, k alike), linear index
 * (k (ny - 1) + j)(nx - 1) + i, has corner c at voxel (i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)); a cell with an unknown
 * corner has no triangle.  tri_count [cells] uint8: the triangles of every cell (0..12), six tetrahedra around the diagonal
 * from corner 0 to corner 7 with one or two triangles each.  min_count >= 1.  One launch, a lane per cell. */
int cloudaae_tsdf_count(int nx, int ny, int nz, const int *state, int min_count, uint8_t *tri_count, cloudaae_stream_t stream);

/* The triangles themselves.  tri_offset [cells] long long: the exclusive prefix sum of cloudaae_tsdf_count's tri_count for the
 * same state and min_count; total: their sum (0: nothing is launched); a cell whose offset and count do not fit into [0,
 * total] writes nothing.  tri_pos [total,3,3] double: the vertices in metres; tri_key [total,3] long long: the vertex's edge,
 * lo * 8 + code, lo the smaller linear voxel index of the edge's two voxels and code = dx + 2 dy + 4 dz of the other minus lo
 * (1..7).  A vertex lies at c_lo + (c_hi - c_lo) t per coordinate, t = v_lo / (v_lo - v_hi): the same bits from every cell
 * that touches the edge.  Order: cell, tetrahedron, triangle; normals (p1 - p0) x (p2 - p0) point from inside to outside.
 * One launch, a lane per cell. */
int cloudaae_tsdf_emit(int nx, int ny, int nz, double ox, double oy, double oz, double voxel, const int *state, int min_count,
                       const long long *tri_offset, long long total, double *tri_pos, long long *tri_key,
                       cloudaae_stream_t stream);

/* The volume seen from a pose, as a uint16 depth window ("Scanning").  B samples; sample b has the window's row
 * intr_win[b] = (fx, fy, cxw, cyw, factor_depth) and poses[b] (4x4 row-major, model -> camera, R and t).  float64 on exactly
 * widened values, un-fused, in the order written; comparisons in float64 before any conversion.  Window pixel (x, y): dx = (x -
 * cxw) / fx, dy = (y - cyw) / fy; the ray is parametrised by the camera depth z.  Per axis a: o_a = -((R0a t0 + R1a t1) + R2a
 * t2), d_a = (R0a dx + R1a dy) + R2a, g0_a = (o_a - origin_a) / voxel - 0.5, gd_a = d_a / voxel: g(z) = g0 + z gd in
 * voxel-centre coordinates.  Interval: z0 = z_near, z1 = 65535 / factor_depth; per axis with n voxels: gd_a == 0 misses unless
 * 0 <= g0_a <= n - 1; else ta = (0 - g0_a) / gd_a, tb = ((n - 1) - g0_a) / gd_a, z0 = max(z0, min(ta, tb)), z1 = min(z1,
 * max(ta, tb)); a NaN misses; the ray misses unless z0 <= z1.  Samples z_k = z0 + (double) k step, k = 0, 1, ... while z_k <=
 * z1 and k < 4096.  At a sample g = g0 + z_k gd; the cell is i_a = clamp(floor g_a, 0, n_a - 2), f_a = g_a - i_a; the eight
 * corner values are cloudaae_tsdf_count's with min_count, the sample is unknown when any is; else trilinear: along x v0 + (v1 -
 * v0) f_x on the corner pairs (0,1), (2,3), (4,5), (6,7), then along y, then along z.  prev starts unknown; an unknown sample
 * sets prev unknown; v >= 0 sets prev = (v, z_k); v < 0 ends the ray, and with a known prev = (v_p, z_p) it is a hit: z* = z_p +
 * (z_k - z_p) (v_p / (v_p - v)), du = floor(z* factor_depth + 0.5), the pixel is du when 1 <= du <= 65535.  Every other pixel
 * is 0; every pixel of depth_out [B,wh,ww] is written.  Limits: the volume's; B, wh, ww >= 1, wh ww <= 2^24, B wh ww <= 2^28;
 * min_count >= 1; step and z_near finite and > 0.  One launch, a lane per pixel, no atomics. */
int cloudaae_tsdf_raycast(int nx, int ny, int nz, double ox, double oy, double oz, double voxel, const int *state, int min_count,
                          int B, int wh, int ww, const float *intr_win, const double *poses, double step, double z_near,
                          uint16_t *depth_out, cloudaae_stream_t stream);

/* One Gauss-Newton step that aligns depth frames on the volume's signed distance field ("Scanning on the field"):
 * no raycast, no second normal map.  The volume, state and min_count as above; front > 0, metres: what a field value of 4096
 * stands for (the front of the integration that made the state).  depth [f,h,w] uint16, label [f,h,w] uint8 and want [f] int
 * (both or neither) as in cloudaae_tsdf_integrate.  b samples: frame_of [b] int, origin [b,2] int = (u0, v0), any values, one
 * window size wh x ww, intr_win [b,5] float = (fx, fy, cx - u0, cy - v0, factor_depth) and pose_in [b,16] double (row-major 4 x
 * 4, model -> camera, R and t) as in cloudaae_depth_align_step.  float64 on exactly widened values, un-fused, in the order
 * written; comparisons in float64 before any conversion.  Window pixel (x, y) of sample s with fr = frame_of[s]: d = the depth
 * of frame fr at (u0 + x, v0 + y), 0 outside the frame; no row when d = 0, or when label and want are given, want[fr] != 0 and
 * the label at that pixel differs.  p = P(x, y, d) of cloudaae_depth_align_step; e = p - t; q_a = (R0a e0 + R1a e1) + R2a e2;
 * g_a = (q_a - origin_a) / voxel - 0.5; no row unless 0 <= g_a <= n_a - 1 on every axis (a NaN fails).  The cell i_a =
 * clamp(floor g_a, 0, n_a - 2), f_a = g_a - i_a and its eight corner values v0..v7 are cloudaae_tsdf_raycast's; no row when a
 * corner is unknown.  c00 = v0 + (v1 - v0) f_x, c10 on (2,3), c01 on (4,5), c11 on (6,7); c0 = c00 + (c10 - c00) f_y, c1 = c01
 * + (c11 - c01) f_y; val = c0 + (c1 - c0) f_z.  The gradient by (f_x, f_y, f_z): with d00 = v1 - v0, d10 = v3 - v2, d01 = v5 -
 * v4, d11 = v7 - v6: gx0 = d00 + (d10 - d00) f_y, gx1 = d01 + (d11 - d01) f_y, G_x = gx0 + (gx1 - gx0) f_z; e0 = c10 - c00, e1 =
 * c11 - c01, G_y = e0 + (e1 - e0) f_z; G_z = c1 - c0.  No row when val >= 4096 or (G_x G_x + G_y G_y) + G_z G_z is 0 or not
 * finite.  r = (val / 4096) front; o = G ((front / 4096) / voxel); n_i = (Ri0 o_0 + Ri1 o_1) + Ri2 o_2; a = p x n formed as in
 * cloudaae_depth_align_step; J = (-a, -n).  The sums, A x = -b by LDL^T, U and pose_out = U pose_in are
 * cloudaae_depth_align_step's.
 * Outputs, all written: n_pairs [b] int: the rows; x [b,6] double (zeros unless status is 0); status [b] int: 0 updated, 1
 * fewer than six rows, 2 a pivot that is not a finite number > 0, 3 a solution that is not finite, 4 frame_of outside [0, f)
 * (nothing of that sample is read; n_pairs is 0); pose_out [b,16] double, for every status but 0 pose_in bit for bit.
 * Two launches, runs of 2048 window pixels, as cloudaae_depth_align_step: no floating-point atomics and no workgroup waits
 * for another, the same bits run to run and whatever else is in the batch.  workspace:
 * cloudaae_tsdf_align_step_workspace(b, wh, ww) bytes, 8-byte aligned (0: outside the limits).  Limits: the volume's;
 * min_count >= 1; front finite and > 0; f, h, w, b, wh, ww >= 1; h * w <= 2^24; wh * ww <= 2^24; b * wh * ww <= 2^28; outside
 * them, with a null required pointer, a state that is not 16-byte aligned or a workspace too small the call returns an error,
 * launches nothing and leaves its outputs untouched. */
long long cloudaae_tsdf_align_step_workspace(int b, int wh, int ww);
int cloudaae_tsdf_align_step(int nx, int ny, int nz, double ox, double oy, double oz, double voxel, const int *state, int min_count,
                             double front, int f, int h, int w, const uint16_t *depth, const uint8_t *label, const int *want,
                             int b, const int *frame_of, const int *origin, int wh, int ww, const float *intr_win,
                             const double *pose_in, int *n_pairs, double *x, int *status, double *pose_out, void *workspace,
                             long long workspace_size, cloudaae_stream_t stream);

/* ---- simplified meshes: uniform vertex clustering with quadric-error placement ("Simplified meshes") ---- */

/* Shared by the four entries below.  The grid has nx x ny x nz cells of side `cell` with its low corner at (ox, oy, oz); the
 * centre of cell (gx, gy, gz) is z = o + (g + 0.5) cell per axis and its key (gz ny + gy) nx + gx.  vertices [V,3] float,
 * triangles [T,3] int.  The cells of a mesh are the distinct keys >= 0 of its vertices in ascending order, a cell's position in
 * that order is its rank; rank [V] int holds every vertex's, -1 for an unused vertex; cell_grid [C,3] int holds (gx, gy, gz)
 * per cell.  A triangle is dropped when an index lies outside [0, V) or a corner's rank is < 0.  All arithmetic is float64 on
 * exactly widened values, un-fused, in the order written; comparisons in float64 before any conversion.  Limits: 0 <= V, T <
 * 2^31 / 3; 0 <= C <= 2^21; the origin finite, cell (and eps) finite and > 0; 1 <= nx, ny, nz <= 2^20.  Outside them, or with
 * a null required pointer, a call returns an error, launches nothing and leaves its outputs untouched; V = 0 (keys), C = 0
 * (sums, place) and T = 0 (triangles) launch nothing and succeed. */

/* key [V] long long: per axis g = floor((p - o) / cell); the vertex's key when 0 <= g < n on every axis (a NaN or an infinity
 * fails: a vertex exactly on a cell's upper plane belongs to the next cell, one on the grid's far plane is outside), else -1.
 * One launch, a lane per vertex. */
int cloudaae_mesh_cluster_keys(int V, const float *vertices, double ox, double oy, double oz, double cell, int nx, int ny, int nz,
                               long long *key, cloudaae_stream_t stream);

/* The sums of every cell.  sums [C,16] double: m [0:3] = sum of q = p - z over the cell's vertices; then over every corner (t,
 * k) of a triangle that is not dropped whose vertex lies in the cell, with q_i = p_i - z of the triangle's three vertices, u =
 * q_1 - q_0, w = q_2 - q_0, n = u x w (n_0 = u_1 w_2 - u_2 w_1, ...), d = -((n_0 q_00 + n_1 q_01) + n_2 q_02): A [3:9] += (n_0
 * n_0, n_0 n_1, n_0 n_2, n_1 n_1, n_1 n_2, n_2 n_2), b [9:12] += n d, e [12] += d d; [13:16] are written as zeros.  counts
 * [C,2] int: the vertices and the corners added.  vert_order [n_vert_order] int: vertices grouped by rank, ascending index
 * inside a group, the group of cell r at [vert_start[r], vert_start[r + 1]); corner_order [n_corner_order] int, corner_start
 * alike for the corners 3 t + k; vert_start, corner_start [C + 1] long long.  A range is cut to its list; an entry that is out
 * of range, or whose vertex (corner) does not belong to the cell, or whose triangle is dropped, is skipped: bad lists read
 * nothing outside the arrays.  n_vert_order <= V, n_corner_order <= 3 T.  A cell's additions: lane l of the cell's wave takes
 * the entries l, l + 64, ... of each range in order, then the 64 lanes meet in a fixed butterfly -- the order follows from the
 * cell's two lists alone.  One launch, a wave per cell, no atomics. */
int cloudaae_mesh_cluster_sums(int V, int T, const float *vertices, const int *triangles, int C, const int *rank,
                               const int *cell_grid, double ox, double oy, double oz, double cell, const int *vert_order,
                               long long n_vert_order, const long long *vert_start, const int *corner_order,
                               long long n_corner_order, const long long *corner_start, double *sums, int *counts,
                               cloudaae_stream_t stream);

/* The vertex of every cell.  mean = m / n_v.  A is eigen-decomposed by 8 sweeps of cyclic Jacobi over the pairs (0,1), (0,2),
 * (1,2); a rotation of (p, q) does nothing when a_pq == 0, else theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| +
 * sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, (a_rp, a_rq) = (c a_rp - s
 * a_rq, s a_rp + c a_rq) and the same for every row of V.  lam_max is the largest diagonal entry; unless all three are finite
 * and lam_max > 0: x = mean, how = 4.  Else r = -b - A mean, x = mean, and for i = 0, 1, 2 with lam_i > eps lam_max: x += v_i
 * ((v_i . r) / lam_i); how = the number of those; if some |x_a| > cell / 2 or x is not finite: x = mean, how += 4.  pos [C,3]
 * double = z + x; how [C] uint8; err [C] double = ((A x) . x + 2 (b . x)) + e, every dot product (t0 + t1) + t2.  One launch, a
 * lane per cell. */
int cloudaae_mesh_cluster_place(int C, const double *sums, const int *counts, const int *cell_grid, double ox, double oy,
                                double oz, double cell, double eps, double *pos, uint8_t *how, double *err,
                                cloudaae_stream_t stream);

/* tri_key [T] long long: -1 when the triangle is dropped, a corner's rank lies outside [0, C), or two of its three ranks are
 * equal; else the ranks rotated so that the smallest comes first (the orientation stays), packed as (r_a 2^21 + r_b) 2^21 +
 * r_c.  One launch, a lane per triangle. */
int cloudaae_mesh_cluster_triangles(int V, int T, const int *triangles, const int *rank, int C, long long *tri_key,
                                    cloudaae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDAAE_HIP_H */
