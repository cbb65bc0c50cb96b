// pose_sample.hip -- training poses and object occluders drawn on the GPU (gfx950).
//
// Replaces the pose side of the reference's on-line synthesis, which this project so far read from pose records:
//   sample_rot / rotation_generation                    utils/sample_pose_in_frustum.py:8-39
//   in_frustum_translation .. translation_generation    utils/sample_pose_in_frustum.py:73-153
//   get_random_object_occluder                          utils/generate_occluder.py:5-35
// DESIGN.md, "Pose sampling", is the definition; tests/pose_sampling_reference.py restates it in NumPy.  Every draw is a
// pure function of (seed, global sample index g, stream id) through philox4x32: the counter is g = first_index + i, so a
// sample does not depend on the batch size, the number of ranks or the launch, and a recorded call replays to the same
// bits.  All fp32 arithmetic is un-fused (the file is compiled with -ffp-contract=off) in the order written here.
#include "common.h"
#include "philox.h"
#include "so3_dual.h"
#include "../../include/cloudaae_hip.h"
#include <math.h>

namespace cloudaae {

// Philox stream ids of this file (synth.hip uses 1, 2, 3, 4 and 7; step.hip's input noise uses the hash of its own draw
// counter as the stream and its own seed, and a counter with the cloud in the high word)
constexpr unsigned PS_STREAM_POSE = 16u;        // r0 class, r1 theta, r2 u, r3 angle
constexpr unsigned PS_STREAM_TRANS = 17u;       // normal2(r0, r1) -> x, y; normal2(r2, r3) -> z, (unused)
constexpr unsigned PS_STREAM_OCC_CENTRE = 18u;  // normal2(r0, r1) -> centre x, y; normal2(r2, r3) -> centre z, (unused)
constexpr unsigned PS_STREAM_OCC_CLASS = 19u;   // r0 class of the occluder

constexpr int PS_MAX_CLASSES = 128;
struct ClassList {             // passed by value: the caller's list is host memory
    int n;
    int id[PS_MAX_CLASSES];
};

struct Camera {
    float wnear, wfar, near_d, far_d, fx, fy, cx, cy, width, height;
};

// uniform over n entries from 32 raw bits: floor(r n / 2^32)
__device__ __forceinline__ int ps_pick(unsigned r, int n) { return (int)(((unsigned long long)r * (unsigned long long)n) >> 32); }

// one lane per sample
__global__ __launch_bounds__(64) void sample_poses_kernel(int b, unsigned long long first, unsigned long long seed,
                                                  ClassList classes, Camera cam, long long *__restrict__ class_id,
                                                  double *__restrict__ axisangle, double *__restrict__ rot,
                                                  float *__restrict__ rot32, float *__restrict__ trans, unsigned char *__restrict__ in_fov,
                                                  float *__restrict__ drawn, unsigned *__restrict__ raw)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b)
        return;
    const unsigned long long g = first + (unsigned long long)i;
    unsigned r[4], q[4];
    philox4x32(seed, g, PS_STREAM_POSE, r);
    philox4x32(seed, g, PS_STREAM_TRANS, q);
    if (raw) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            raw[8 * i + k] = r[k];
            raw[8 * i + 4 + k] = q[k];
        }
    }
    class_id[i] = (long long)classes.id[ps_pick(r[0], classes.n)];
    // sample_rot (:8-27): a point of the unit sphere, times an angle
    const float theta = 6.283185307179586f * u01(r[1]);
    const float u = 2.0f * u01(r[2]) - 1.0f;
    const float s = sqrtf(1.0f - u * u);
    const float ax = s * cosf(theta), ay = s * sinf(theta), az = u;
    const float angle = 3.14159265358979f * (2.0f * u01(r[3]) - 1.0f);
    const float a32[3] = {ax * angle, ay * angle, az * angle};
    Dual a[3], M[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        axisangle[3 * i + k] = (double)a32[k];
        a[k] = dconst((double)a32[k]);
    }
    exp_map(a, M);
    for (int rr = 0; rr < 3; ++rr)
        for (int c = 0; c < 3; ++c)
        {
            rot[9 * i + 3 * rr + c] = M[rr][c].v;
            if (rot32)
                rot32[9 * i + 3 * rr + c] = (float)M[rr][c].v;      // rot_gen_mat (:35): the cast of the reference
        }
    // in_frustum_translation (:73-82) and get_final_translation (:119-124)
    float n0, n1, n2, n3;
    normal2(q[0], q[1], n0, n1);
    normal2(q[2], q[3], n2, n3);
    const float sxy = (cam.wnear + cam.wfar) / 7.0f;
    const float zmid = (cam.far_d + cam.near_d) / 2.0f;
    const float sz = (cam.far_d - cam.near_d) / 7.0f;
    const float x = n0 * sxy, y = n1 * sxy, z = zmid + n2 * sz;
    const float pu = (cam.fx * x + cam.cx * z) / z, pv = (cam.fy * y + cam.cy * z) / z;
    const bool keep = (pu > 0.0f && pu < cam.width) && (pv > 0.0f && pv < cam.height);
    trans[3 * i] = keep ? x : 0.0f;
    trans[3 * i + 1] = keep ? y : 0.0f;
    trans[3 * i + 2] = keep ? z : zmid;
    in_fov[i] = keep ? 1 : 0;
    if (drawn) {
        drawn[5 * i] = x;
        drawn[5 * i + 1] = y;
        drawn[5 * i + 2] = z;
        drawn[5 * i + 3] = pu;
        drawn[5 * i + 4] = pv;
    }
}

// The object occluder of global sample g whose target lies at depth z: its class (the return value) and its centre c,
// with the raw words r (centre) and q (class).  The one place of the rule: cloudaae_random_object_occluder and
// cloudaae_rendered_scene both draw through it.
__device__ __forceinline__ int ps_occluder_draw(unsigned long long seed, unsigned long long g, const ClassList &classes,
                                                float z, float wnear, float hnear, float near_d, unsigned (&r)[4],
                                                unsigned (&q)[4], float (&c)[3])
{
    philox4x32(seed, g, PS_STREAM_OCC_CENTRE, r);
    philox4x32(seed, g, PS_STREAM_OCC_CLASS, q);
    float n0, n1, n2, n3;
    normal2(r[0], r[1], n0, n1);
    normal2(r[2], r[3], n2, n3);
    c[0] = n0 * (wnear / 8.0f);
    c[1] = n1 * (hnear / 8.0f);
    c[2] = (near_d + z) / 2.0f + n2 * ((z - near_d) / 6.0f);
    return classes.id[ps_pick(q[0], classes.n)];
}

// get_random_object_occluder (generate_occluder.py:5-35): one lane per (sample, point).  The centre and the class are
// functions of the sample alone, so every lane of a sample derives the same ones.
__global__ __launch_bounds__(256) void object_occluder_kernel(int b, unsigned long long first, unsigned long long seed,
                                                      int npts, const float *__restrict__ models, ClassList classes,
                                                      const double *__restrict__ rot, const float *__restrict__ trans,
                                                      int per, float wnear, float hnear, float near_d,
                                                      float *__restrict__ occ, long long *__restrict__ occ_class,
                                                      unsigned *__restrict__ raw)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b * per)
        return;
    const int cloud = i / per, j = i - cloud * per;
    unsigned r[4], q[4];
    float c[3];
    const int cls = ps_occluder_draw(seed, first + (unsigned long long)cloud, classes, trans[cloud * 3 + 2], wnear, hnear,
                                     near_d, r, q, c);
    if (j == 0) {
        if (occ_class)
            occ_class[cloud] = (long long)cls;
        if (raw) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                raw[8 * cloud + k] = r[k];
                raw[8 * cloud + 4 + k] = q[k];
            }
        }
    }
    const float *p = models + ((size_t)cls * npts + j) * 6;
    const double *R = rot + (size_t)cloud * 9;
    // the dot product of transform_model_kernel (synth.hip): float32(R), left to right, un-fused
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        const float r0 = (float)R[3 * rr], r1 = (float)R[3 * rr + 1], r2 = (float)R[3 * rr + 2];
        const float a = p[0] * r0, bb = p[1] * r1, cc = p[2] * r2;
        occ[(size_t)i * 3 + rr] = ((a + bb) + cc) + c[rr];
    }
}

// [R | t; 0 0 0 1], row-major: the model -> camera pose the renderer takes
__device__ __forceinline__ void ps_pose(const double *__restrict__ R, double tx, double ty, double tz,
                                        double *__restrict__ out)
{
    const double t[3] = {tx, ty, tz};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        out[4 * rr + 0] = R[3 * rr + 0];
        out[4 * rr + 1] = R[3 * rr + 1];
        out[4 * rr + 2] = R[3 * rr + 2];
        out[4 * rr + 3] = t[rr];
    }
    out[12] = 0.0, out[13] = 0.0, out[14] = 0.0, out[15] = 1.0;
}

// The scene of a rendered training batch ("Rendered training clouds"): one lane per sample writes the three
// instances of its two frames.  Frame 2i holds instance 3i (the target alone); frame 2i + 1 holds 3i + 1 (the target
// again) and 3i + 2 (the occluder: the class and the centre of ps_occluder_draw, under the sample's own rotation).  The
// classes live on the device, so instance j's vertex and triangle ranks start at j * max_v and j * max_t; the renderer
// treats the ranks past a mesh's own counts as absent.  A class outside mesh_index gives mesh -1: nothing is drawn.
__global__ __launch_bounds__(64) void rendered_scene_kernel(int b, unsigned long long first, unsigned long long seed,
                                                           ClassList classes, int nmodels,
                                                           const long long *__restrict__ class_id,
                                                           const int *__restrict__ mesh_index,
                                                           const double *__restrict__ rot, const float *__restrict__ trans,
                                                           float wnear, float hnear, float near_d, int max_v, int max_t,
                                                           int *__restrict__ inst_offsets, int *__restrict__ inst_mesh,
                                                           int *__restrict__ inst_label, double *__restrict__ inst_pose,
                                                           int *__restrict__ vert_base, int *__restrict__ tri_base,
                                                           long long *__restrict__ occ_class, float *__restrict__ occ_centre)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b)
        return;
    unsigned r[4], q[4];
    float c[3];
    const float *t = trans + 3 * (size_t)i;
    const int ocls = ps_occluder_draw(seed, first + (unsigned long long)i, classes, t[2], wnear, hnear, near_d, r, q, c);
    const long long cls = class_id[i];
    const int target = (cls >= 0 && cls < nmodels) ? mesh_index[cls] : -1;
    const int occluder = mesh_index[ocls];         // (the class list was checked against nmodels by the host)
    const double *R = rot + 9 * (size_t)i;
    const int j = 3 * i;
    inst_offsets[2 * i] = j;
    inst_offsets[2 * i + 1] = j + 1;
    inst_mesh[j] = target, inst_mesh[j + 1] = target, inst_mesh[j + 2] = occluder;
    inst_label[j] = 1, inst_label[j + 1] = 1, inst_label[j + 2] = 2;
    ps_pose(R, (double)t[0], (double)t[1], (double)t[2], inst_pose + 16 * (size_t)j);
    ps_pose(R, (double)t[0], (double)t[1], (double)t[2], inst_pose + 16 * (size_t)(j + 1));
    ps_pose(R, (double)c[0], (double)c[1], (double)c[2], inst_pose + 16 * (size_t)(j + 2));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vert_base[j + k] = (j + k) * max_v;
        tri_base[j + k] = (j + k) * max_t;
    }
    occ_class[i] = (long long)ocls;
    if (occ_centre) {
        occ_centre[3 * i + 0] = c[0];
        occ_centre[3 * i + 1] = c[1];
        occ_centre[3 * i + 2] = c[2];
    }
    if (i == b - 1) {
        inst_offsets[2 * b] = 3 * b;
        vert_base[3 * b] = 3 * b * max_v;
        tri_base[3 * b] = 3 * b * max_t;
    }
}

// the caller's class list (host memory; null with n = 0: every model) -> the by-value list of a launch; the message of
// the first rule it breaks, or null
static const char *ps_class_list(int n_classes, const int *classes, int nmodels, ClassList &out)
{
    if (nmodels < 1)
        return "nmodels must be >= 1";
    if (classes == nullptr && n_classes != 0)
        return "null pointer";
    if (classes != nullptr && n_classes < 1)
        return "empty class list";
    const int n = classes ? n_classes : nmodels;
    if (n > PS_MAX_CLASSES)
        return "class list longer than 128";
    out.n = n;
    for (int k = 0; k < n; ++k) {
        const int c = classes ? classes[k] : k;
        if (c < 0 || c >= nmodels)
            return "class id outside the models";
        out.id[k] = c;
    }
    return nullptr;
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_sample_poses(int b, unsigned long long first_index, unsigned long long seed, int n_classes,
                                       const int *classes, int nmodels, float wnear, float wfar, float near_dist,
                                       float far_dist, float fx, float fy, float cx, float cy, float width, float height,
                                       long long *class_id, double *axisangle, double *rot_mat64, float *rot_mat32,
                                       float *translation, unsigned char *in_fov, float *drawn, unsigned *raw,
                                       cloudaae_stream_t stream)
{
    const char *name = "cloudaae_sample_poses";
    CLOUDAAE_REQUIRE(b >= 1, name, "b must be >= 1");
    CLOUDAAE_REQUIRE(class_id && axisangle && rot_mat64 && translation && in_fov, name, "null pointer");
    ClassList list;
    const char *bad = ps_class_list(n_classes, classes, nmodels, list);
    CLOUDAAE_REQUIRE(bad == nullptr, name, bad);
    CLOUDAAE_REQUIRE(far_dist > near_dist && isfinite(far_dist) && isfinite(near_dist), name, "far must be > near");
    CLOUDAAE_REQUIRE(width > 0.0f && height > 0.0f, name, "width and height must be > 0");
    CLOUDAAE_REQUIRE(isfinite(wnear) && isfinite(wfar) && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy), name,
                     "camera constants must be finite");
    const Camera cam = {wnear, wfar, near_dist, far_dist, fx, fy, cx, cy, width, height};
    hipLaunchKernelGGL(sample_poses_kernel, dim3(ceil_div(b, 64)), dim3(64), 0, (hipStream_t)stream, b, first_index, seed, list,
                       cam, class_id, axisangle, rot_mat64, rot_mat32, translation, in_fov, drawn, raw);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_random_object_occluder(int b, unsigned long long first_index, unsigned long long seed, int nmodels,
                                                 int npts, const float *models, int n_classes, const int *classes,
                                                 const double *rot_mat64, const float *translation, int per, float wnear,
                                                 float hnear, float near_dist, float *occluder, long long *occ_class,
                                                 unsigned *raw, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_random_object_occluder";
    CLOUDAAE_REQUIRE(b >= 1, name, "b must be >= 1");
    CLOUDAAE_REQUIRE(per >= 1, name, "per must be >= 1");
    CLOUDAAE_REQUIRE(npts >= 1 && per <= npts, name, "per above the model's points");
    CLOUDAAE_REQUIRE((long long)b * per <= (1ll << 30), name, "b * per above the limit of 2^30 points");
    CLOUDAAE_REQUIRE(models && rot_mat64 && translation && occluder, name, "null pointer");
    ClassList list;
    const char *bad = ps_class_list(n_classes, classes, nmodels, list);
    CLOUDAAE_REQUIRE(bad == nullptr, name, bad);
    CLOUDAAE_REQUIRE(isfinite(wnear) && isfinite(hnear) && isfinite(near_dist), name, "camera constants must be finite");
    hipLaunchKernelGGL(object_occluder_kernel, dim3(ceil_div((long long)b * per, 256)), dim3(256), 0, (hipStream_t)stream, b,
                       first_index, seed, npts, models, list, rot_mat64, translation, per, wnear, hnear, near_dist, occluder,
                       occ_class, raw);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_rendered_scene(int b, unsigned long long first_index, unsigned long long seed, int nmodels,
                                         int n_classes, const int *classes, const long long *class_id, const int *mesh_index,
                                         const double *rot_mat64, const float *translation, float wnear, float hnear,
                                         float near_dist, int max_vertices, int max_triangles, int *inst_offsets,
                                         int *inst_mesh, int *inst_label, double *inst_pose, int *inst_vert_base,
                                         int *inst_tri_base, long long *occ_class, float *occ_centre, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_rendered_scene";
    CLOUDAAE_REQUIRE(b >= 1, name, "b must be >= 1");
    CLOUDAAE_REQUIRE(max_vertices >= 1 && max_triangles >= 1, name, "max_vertices and max_triangles must be >= 1");
    CLOUDAAE_REQUIRE(3ll * b * max_vertices <= 2147483647ll && 3ll * b * max_triangles <= 2147483647ll, name,
                     "3 b max_vertices and 3 b max_triangles (the strided ranks) must lie below 2^31");
    CLOUDAAE_REQUIRE(class_id && mesh_index && rot_mat64 && translation && inst_offsets && inst_mesh && inst_label &&
                         inst_pose && inst_vert_base && inst_tri_base && occ_class,
                     name, "null pointer");
    ClassList list;
    const char *bad = ps_class_list(n_classes, classes, nmodels, list);
    CLOUDAAE_REQUIRE(bad == nullptr, name, bad);
    CLOUDAAE_REQUIRE(isfinite(wnear) && isfinite(hnear) && isfinite(near_dist), name, "camera constants must be finite");
    hipLaunchKernelGGL(rendered_scene_kernel, dim3(ceil_div(b, 64)), dim3(64), 0, (hipStream_t)stream, b, first_index, seed, list,
                       nmodels, class_id, mesh_index, rot_mat64, translation, wnear, hnear, near_dist, max_vertices,
                       max_triangles, inst_offsets, inst_mesh, inst_label, inst_pose, inst_vert_base, inst_tri_base, occ_class,
                       occ_centre);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
