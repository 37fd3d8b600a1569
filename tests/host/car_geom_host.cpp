// Host shim for CPU-side unit tests of cross_attention_renderer_amd/csrc/car_geom.h (test infrastructure).
// Compiled by g++ (tests/test_geom_host.py) with -ffp-contract=off; it loops the very same inline
// functions the HIP kernels call, so the geometry can be checked against the oracle without a GPU.
#include "car_geom.h"

extern "C" {

void host_pose_setup(const float* c2w_ctx, const float* c2w_q, const float* K_ctx, const float* K_q,
                     int b, int V, int H, CarPose* out) {
    for (int i = 0; i < b; ++i)
        car_pose_setup(c2w_ctx + 16 * V * i, c2w_q + 16 * i, K_ctx + 16 * V * i, K_q + 16 * i, V, H, out + V * i);
}

void host_ray_setup(const CarPose* poses, const float* uv, int b, int V, int R, CarRay* out) {
    for (int n = 0; n < b * V; ++n)
        for (int r = 0; r < R; ++r) {
            const float* p = uv + 2 * ((n / V) * R + r);
            car_ray_setup(poses[n], p[0], p[1], out + (size_t)n * R + r);
        }
}

void host_sample_setup(const CarPose* poses, const CarRay* rays, const float* interval, int b, int V, int R,
                       int P, int H, int W, CarSample* out) {
    for (int n = 0; n < b * V; ++n)
        for (int r = 0; r < R; ++r) {
            const CarRay& ray = rays[(size_t)n * R + r];
            for (int p = 0; p < P; ++p) {
                CarSample* S = out + ((size_t)n * R + r) * P + p;
                for (int i = 0; i < 2; ++i) S->grid[i] = ray.start[i] + (ray.end[i] - ray.start[i]) * interval[p];
                car_sample_setup(poses[n], poses + (n / V) * V, ray, V, H, W, S);
            }
        }
}

// no_sample = 1 (sample_kernel of csrc/car_geometry.hip, the fused kernel's own geometry): a sample is the projection of the query ray's
// point at depth steps[p]
void host_sample_setup_depth(const CarPose* poses, const CarRay* rays, const float* steps, int b, int V, int R,
                             int P, int H, int W, CarSample* out) {
    for (int n = 0; n < b * V; ++n)
        for (int r = 0; r < R; ++r) {
            const CarRay& ray = rays[(size_t)n * R + r];
            const CarPose& Ps = poses[n];
            for (int p = 0; p < P; ++p) {
                CarSample* S = out + ((size_t)n * R + r) * P + p;
                const float s = steps[p];
                const float q[3] = {Ps.q_rel[3] + s * ray.d[0], Ps.q_rel[7] + s * ray.d[1], Ps.q_rel[11] + s * ray.d[2]};
                car_project_grid(Ps.kc, q, H, W, S->grid);
                car_sample_setup(Ps, poses + (n / V) * V, ray, V, H, W, S);
            }
        }
}

// host_ray_setup_depth, host_xenc, host_project_points and host_exchange_rows below are HAND COPIES of kernel bodies of csrc/car_geometry.hip
// (the loops around the header's functions live in the kernels, not in car_geom.h).  A CPU test through them pins the header's functions
// they call and this copy of the loop — not the kernel's own loop, index arithmetic or strict comparisons: only tests/test_geometry_hip.py,
// which runs the kernels against the same restatement, pins those.
// no_sample = 1 of ray_kernel (csrc/car_geometry.hip): uniform depths on the query ray; overlaps = some sample strictly inside; the first and
// the last sample are start and end
void host_ray_setup_depth(const CarPose* poses, const float* uv, const float* depth_steps, int b, int V, int R, int H, int W, int P,
                          CarRay* out) {
    for (int n = 0; n < b * V; ++n)
        for (int r = 0; r < R; ++r) {
            const CarPose& Ps = poses[n];
            const float* p2 = uv + 2 * ((n / V) * R + r);
            CarRay ray;
            car_pixel_ray(Ps.q_rel, Ps.kq, p2[0], p2[1], ray.d, ray.m);
            const float o[3] = {Ps.q_rel[3], Ps.q_rel[7], Ps.q_rel[11]};
            bool any_in = false;
            float first[2] = {0, 0}, last[2] = {0, 0};
            for (int p = 0; p < P; ++p) {
                const float s = depth_steps[p];
                const float q[3] = {o[0] + s * ray.d[0], o[1] + s * ray.d[1], o[2] + s * ray.d[2]};
                float gg[2];
                car_project_grid(Ps.kc, q, H, W, gg);
                any_in = any_in || (gg[0] < 1.0f && gg[0] > -1.0f && gg[1] < 1.0f && gg[1] > -1.0f);
                if (p == 0) { first[0] = gg[0]; first[1] = gg[1]; }
                last[0] = gg[0]; last[1] = gg[1];
            }
            ray.start[0] = first[0]; ray.start[1] = first[1];
            ray.end[0] = last[0]; ray.end[1] = last[1];
            ray.overlaps = any_in ? 1.0f : 0.0f;
            ray.pad = 0.0f;
            out[(size_t)n * R + r] = ray;
        }
}

// the xenc window of sample_kernel: V == 1: tanh(pt / 5), tanh(pt / 100) (6 wide); otherwise tanh(pt_in[s] / 5) per view (3 wide)
void host_xenc(const CarSample* samples, long n, int V, float* xenc) {
    for (long i = 0; i < n; ++i) {
        const CarSample& S = samples[i];
        if (V == 1) {
            for (int k = 0; k < 3; ++k) { xenc[6 * i + k] = tanhf(S.pt[k] / 5.0f); xenc[6 * i + 3 + k] = tanhf(S.pt[k] / 100.0f); }
        } else {
            for (int s = 0; s < V; ++s)
                for (int k = 0; k < 3; ++k) xenc[(i * V + s) * 3 + k] = tanhf(S.pt_in[s][k] / 5.0f);
        }
    }
}

// project_points_kernel
void host_project_points(const CarPose* poses, const float* pts, int n_scenes, long npts, int V, int view, int H, int W, float* grid) {
    for (long i = 0; i < (long)n_scenes * npts; ++i) {
        const int sc = (int)(i / npts);
        car_project_grid(poses[sc * V + view].kc, pts + 3 * i, H, W, grid + 2 * i);
    }
}

// exchange_rows_kernel
void host_exchange_rows(const CarPose* poses, const float* pixel_val, const float* pt_in, const float* ptenc, int n_scenes, int V, long pts,
                        int H, int W, int* row_src, float* row_grid, float* row_pe) {
    for (long idx = 0; idx < (long)n_scenes * V * pts * V; ++idx) {
        const int k = (int)(idx % V);
        const long sj = idx / V;
        const long j = sj % pts;
        const int n = (int)(sj / pts), c = n % V, sc = n / V;
        const int o = k == 0 ? c : (k - 1 < c ? k - 1 : k);
        const long so = ((long)(sc * V + o) * pts + j);
        float g2[2];
        if (k == 0) { g2[0] = pixel_val[2 * so]; g2[1] = pixel_val[2 * so + 1]; }
        else car_project_grid(poses[sc * V + o].kc, pt_in + (so * V + c) * 3, H, W, g2);
        row_src[idx] = (sc * V + o) | (k == 0 ? 0 : (1 << 30));
        row_grid[2 * idx] = g2[0]; row_grid[2 * idx + 1] = g2[1];
        const float* pe = ptenc + (so * V + c) * 4;
        row_pe[4 * idx] = pe[0]; row_pe[4 * idx + 1] = pe[1]; row_pe[4 * idx + 2] = pe[2]; row_pe[4 * idx + 3] = 0.0f;
    }
}

void host_bilinear_taps(const float* grid, int n, int W, int H, int mode, int* idx, float* w) {
    for (int i = 0; i < n; ++i) car_bilinear_taps(grid[2 * i], grid[2 * i + 1], W, H, mode, idx + 4 * i, w + 4 * i);
}

// the merged lattice as car_project_maps' merge kernel builds it (csrc/car_lattice.hip merge_kernel): levels [n][h][w][C], r = how
// many times coarser than the widest level; lat [2 modes][lh][lw][C]
void host_lattice_build(const float* const* g, const int* h, const int* w, const int* r, int n_levels, int C, int lh, int lw, int pad, float* lat) {
    for (int mode = 0; mode < 2; ++mode)
        for (int jy = 0; jy < lh; ++jy)
            for (int jx = 0; jx < lw; ++jx) {
                float* o = lat + (((size_t)mode * lh + jy) * lw + jx) * C;
                for (int c = 0; c < C; ++c) o[c] = 0.0f;
                for (int l = n_levels - 1; l >= 0; --l) {
                    const float r2 = (float)(2 * r[l]);
                    int t4[4];
                    float w4[4];
                    car_bilinear_taps_px((float)(jx - pad + 1 - r[l]) / r2, (float)(jy - pad + 1 - r[l]) / r2, w[l], h[l], mode, t4, w4);
                    for (int t = 0; t < 4; ++t)
                        for (int c = 0; c < C; ++c) o[c] = fmaf(w4[t], g[l][(size_t)t4[t] * C + c], o[c]);
                }
            }
}
void host_lattice_taps(const float* grid, int n, int lw, int lh, int pad, float sx, float sy, int* node, int* flags, float* w) {
    for (int i = 0; i < n; ++i) car_lattice_taps(grid[2 * i], grid[2 * i + 1], lw, lh, pad, sx, sy, node + i, flags + i, w + 4 * i);
}

int host_sizeof_pose() { return (int)sizeof(CarPose); }
int host_sizeof_ray() { return (int)sizeof(CarRay); }
int host_sizeof_sample() { return (int)sizeof(CarSample); }
}
