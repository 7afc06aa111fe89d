// sky_taps.h -- the ray and tap arithmetic of the sky cube-map lookup, shared by sky.hip and sky_det.hip: the direction -> face / texel mapping with its
// four bilinear taps and the pinhole ray of a pixel.  The forward, the default backward and the deterministic backward must
// agree on every texel index and weight, so all three call these.  Device code; every includer gets its own copy.
#pragma once
#include "common.h"
#include "device_utils.h"

namespace {

struct Tap { uint32_t idx[4]; float w[4]; };

// direction -> face, (u, v) in [0,1]
__device__ __forceinline__ int index_cube(float x, float y, float z, float& u, float& v) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    int face;
    float c, sc, tc;
    if (az > fmaxf(ax, ay)) { c = z; face = 4; sc = c > 0.f ? x : -x; tc = -y; }
    else if (ay > ax)       { c = y; face = 2; sc = x; tc = c > 0.f ? z : -z; }
    else                    { c = x; face = 0; sc = c > 0.f ? -z : z; tc = -y; }
    if (c < 0.f) face += 1;
    const float m = 0.5f / fabsf(c);
    u = fminf(fmaxf(sc * m + 0.5f, 0.f), 1.f);
    v = fminf(fmaxf(tc * m + 0.5f, 0.f), 1.f);
    return face;
}

__device__ __forceinline__ void face_uv_to_dir(int face, float u, float v, float& x, float& y, float& z) {
    const float s = 2.f * u - 1.f, t = 2.f * v - 1.f;
    switch (face) {
        case 0: x = 1.f;  y = -t;  z = -s;  break;
        case 1: x = -1.f; y = -t;  z = s;   break;
        case 2: x = s;    y = 1.f; z = t;   break;
        case 3: x = s;    y = -1.f; z = -t; break;
        case 4: x = s;    y = -t;  z = 1.f; break;
        default: x = -s;  y = -t;  z = -1.f; break;
    }
}

__device__ __forceinline__ void cube_taps(float dx, float dy, float dz, int res, Tap& tp) {
    float u, v;
    const int face = index_cube(dx, dy, dz, u, v);
    const float uu = u * (float)res - 0.5f, vv = v * (float)res - 0.5f;
    const float fu0 = floorf(uu), fv0 = floorf(vv);
    const float fu = uu - fu0, fv = vv - fv0;
    const int iu0 = (int)fu0, iv0 = (int)fv0;
    const float eps = 0.25f / (float)res;
    float wsum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int iu = iu0 + (k & 1), iv = iv0 + (k >> 1);
        float w = ((k & 1) ? fu : 1.f - fu) * ((k >> 1) ? fv : 1.f - fv);
        const bool out_u = iu < 0 || iu >= res, out_v = iv < 0 || iv >= res;
        int ff = face, ju = iu, jv = iv;
        if (out_u && out_v) { w = 0.f; ff = 0; ju = 0; jv = 0; }        // cube corner: this tap does not exist
        else if (out_u || out_v) {
            // texel centre of the tap with the coordinate that left the face pushed just beyond the edge, re-indexed
            const float tu = iu < 0 ? -eps : (iu >= res ? 1.f + eps : ((float)iu + 0.5f) / (float)res);
            const float tv = iv < 0 ? -eps : (iv >= res ? 1.f + eps : ((float)iv + 0.5f) / (float)res);
            float x, y, z, u2, v2;
            face_uv_to_dir(face, tu, tv, x, y, z);
            ff = index_cube(x, y, z, u2, v2);
            ju = min(max((int)floorf(u2 * (float)res), 0), res - 1);
            jv = min(max((int)floorf(v2 * (float)res), 0), res - 1);
        }
        tp.idx[k] = (uint32_t)((ff * res + jv) * res + ju);
        tp.w[k] = w;
        wsum += w;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) tp.w[k] = tp.w[k] / wsum;
}

// ray of pixel (px, py): get_rays_torch (S3Gaussian/utils/graphics_utils.py:220-241), same operation order
__device__ __forceinline__ void pixel_ray(const EmdSkyArgs& a, int px, int py, size_t p, float& dx, float& dy, float& dz) {
    if (a.dirs) { dx = a.dirs[3 * p]; dy = a.dirs[3 * p + 1]; dz = a.dirs[3 * p + 2]; return; }
    const float ox = a.jitter ? a.jitter[2 * p] : 0.5f, oy = a.jitter ? a.jitter[2 * p + 1] : 0.5f;
    const float X = (float)px + ox, Y = (float)py + oy;
    const float* Ki = a.camera_dev ? a.camera_dev : a.Kinv;           // (device copy of the 21 floats: a recorded pass serves every camera)
    const float* R = a.camera_dev ? a.camera_dev + 9 : a.R; const float* T = a.camera_dev ? a.camera_dev + 18 : a.T;
    // pixel_camera = (X, Y, 1) Kinv^T ; pixel_world = (pixel_camera - T) R ; rays_o = -(R^T T)
    float pc[3], ro[3], pw[3];
#pragma unroll
    for (int k = 0; k < 3; k++) pc[k] = (X * Ki[3 * k] + Y * Ki[3 * k + 1]) + Ki[3 * k + 2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        pw[k] = ((pc[0] - T[0]) * R[k] + (pc[1] - T[1]) * R[3 + k]) + (pc[2] - T[2]) * R[6 + k];
        ro[k] = -((R[k] * T[0] + R[3 + k] * T[1]) + R[6 + k] * T[2]);
    }
    const float rx = pw[0] - ro[0], ry = pw[1] - ro[1], rz = pw[2] - ro[2];
    const float n = sqrtf((rx * rx + ry * ry) + rz * rz);
    dx = rx / n; dy = ry / n; dz = rz / n;
}

}  // namespace
