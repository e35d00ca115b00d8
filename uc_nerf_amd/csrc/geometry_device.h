// The geometry the kernels share.
// Projection: world point -> camera (with the clamp on |cz|) -> pixel, utils/utils.py:333-367 of the reference, for the point and ray kernels
// (render.hip, rays.hip) and the channel-last gathers (gather_cl.hip, mlp_bf16.hip).
// One axis of a (bi|tri)linear grid_sample footprint, for every kernel that interpolates a volume, a map or a source view: the planar gather
// (gather.hip), the channel-last gather (gather_cl.hip) and the gather fused into the split-MLP kernel (mlp_bf16.hip).  grid_sample restated:
//   align_corners=False: i = ((g+1)*size - 1)/2;  align_corners=True: i = (g+1)/2*(size-1);
//   border padding: clamp i to [0, size-1] before floor/frac; a corner index == size gets weight 0.
// Indices count ELEMENTS; plane arithmetic (size_t planes, 32-bit byte offsets) is layout and stays with the kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace ucnerf {

// world -> camera by the 3x4 M; a depth within 1e-4 of the camera plane is moved to 1e-4 (the reference's clamp, sign dropped as there)
__device__ __forceinline__ void to_camera(const float* M, float x, float y, float z, float* cx, float* cy, float* cz) {
    *cx = x * M[0] + y * M[1] + z * M[2] + M[3];
    *cy = x * M[4] + y * M[5] + z * M[6] + M[7];
    float c = x * M[8] + y * M[9] + z * M[10] + M[11];
    if (fabsf(c) < 1e-4f) c = 1e-4f;
    *cz = c;
}

// camera -> homogeneous pixel by the 3x3 K
__device__ __forceinline__ void apply_intrinsics(const float* K, float cx, float cy, float cz, float* qx, float* qy, float* qz) {
    *qx = cx * K[0] + cy * K[1] + cz * K[2];
    *qy = cx * K[3] + cy * K[4] + cz * K[5];
    *qz = cx * K[6] + cy * K[7] + cz * K[8];
}

// world -> homogeneous pixel
__device__ __forceinline__ void project(const float* M, const float* K, float x, float y, float z, float* qx, float* qy, float* qz) {
    float cx, cy, cz;
    to_camera(M, x, y, z, &cx, &cy, &cz);
    apply_intrinsics(K, cx, cy, cz, qx, qy, qz);
}

// project() in one body, for the channel-last gathers (gather_cl.hip, mlp_bf16.hip).  Same values; written out because composed of the two
// functions it changes the code of every feat_gather_cl_kernel, and in one body it changes the ray builders (profiles/geometry_header.md)
__device__ __forceinline__ void project_cl(const float* M, const float* K, float x, float y, float z, float* qx, float* qy, float* qz) {
    const float cx = x * M[0] + y * M[1] + z * M[2] + M[3];
    const float cy = x * M[4] + y * M[5] + z * M[6] + M[7];
    float cz = x * M[8] + y * M[9] + z * M[10] + M[11];
    if (fabsf(cz) < 1e-4f) cz = 1e-4f;
    *qx = cx * K[0] + cy * K[1] + cz * K[2];
    *qy = cx * K[3] + cy * K[4] + cz * K[5];
    *qz = cx * K[6] + cy * K[7] + cz * K[8];
}

// normalised [0,1] coordinate -> grid_sample's [-1,1]
__device__ __forceinline__ float to_grid(float u) { return u * 2.f - 1.0f; }

__device__ __forceinline__ float unnorm(float g, int size, bool align) {
    float i = align ? (g + 1.f) / 2.f * (float)(size - 1) : ((g + 1.f) * (float)size - 1.f) / 2.f;
    return fminf(fmaxf(i, 0.f), (float)(size - 1));
}

struct Lerp {        // one axis of a footprint
    int i0, i1;      // corner indices (i1 clamped into range; its weight is 0 when it was out of range)
    float w0, w1;
};

__device__ __forceinline__ Lerp axis(float g, int size, bool align) {
    const float x = unnorm(g, size, align);
    const float f = floorf(x);
    Lerp a;
    a.i0 = (int)f;
    a.w1 = x - f;
    a.w0 = 1.f - a.w1;
    a.i1 = a.i0 + 1;
    if (a.i1 > size - 1) { a.i1 = size - 1; a.w1 = 0.f; }
    return a;
}

}  // namespace ucnerf
