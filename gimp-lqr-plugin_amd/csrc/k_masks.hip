// k_masks.hip -- E2 for computed masks (include/lqr_masks.h): liblqr's lqr_carver_bias_add_area / _xy and lqr_carver_rigmask_add_area /
// _xy on the bias0 / rig0 planes of a flat carver's base layout.  One-off passes: a thread per pixel, rows of 256 as k_mask_add.
// Every operation is rounded to its C type, as an SSE2 build of liblqr rounds it: the product and the halving in double, one
// conversion to float, one float addition.
#include "lqr_common.h"
#include "lqr_kernels.h"

// bias:     plane[o] += (gfloat) ((gdouble) bias_factor * v / 2)        (lqr_carver_bias.c: lqr_carver_bias_add_area)
// rigidity: plane[o]  = (gfloat) v                                      (lqr_carver_rigmask.c: lqr_carver_rigmask_add_area)
// The mask is mw values wide; (x0, y0) = min(0, offset), (x1, y1) = max(0, offset), nx x ny = the clipped area, all in image orientation;
// a transposed carver's frame is written column by column (strided: fine for a pass that runs once per mask).
template <class T>
__global__ __launch_bounds__(256) void k_mask_add_f(float *plane, int w0, const T *mask, int mw, int x0, int y0, int x1, int y1, int nx, int ny,
                                                    int transposed, int is_rig, int bias_factor)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= nx || y >= ny) return;
    const double v = (double) mask[(size_t) (y - y0) * mw + (x - x0)];      // (float -> double is exact)
    const int xc = transposed ? y + y1 : x + x1;
    const int yc = transposed ? x + x1 : y + y1;
    const size_t o = (size_t) yc * w0 + xc;
    if (is_rig)
        plane[o] = __double2float_rn(v);
    else
        plane[o] = __fadd_rn(plane[o], __double2float_rn(__ddiv_rn(__dmul_rn((double) bias_factor, v), 2.0)));
}
template __global__ void k_mask_add_f<float>(float *, int, const float *, int, int, int, int, int, int, int, int, int, int);
template __global__ void k_mask_add_f<double>(float *, int, const double *, int, int, int, int, int, int, int, int, int, int);

// One bucket of a queued run of _xy calls (host/lqr_mask_queue.h): n entries on n DISTINCT pixels, so no two threads meet.
// bias:     plane[index] += (gfloat) value / 2                          (lqr_carver_bias_add_xy)
// rigidity: plane[index] += (gfloat) value                              (lqr_carver_rigmask_add_xy: it ADDS, unlike the area forms)
__global__ __launch_bounds__(256) void k_mask_scatter(float *plane, const int *index, const double *value, size_t n, int is_rig)
{
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t) index[i];
    const float f = __double2float_rn(value[i]);
    plane[o] = __fadd_rn(plane[o], is_rig ? f : __fdiv_rn(f, 2.0f));
}

// read-out of a plane of a transposed carver in image orientation: out (h0 wide, w0 rows) = plane (w0 wide, h0 rows) transposed
__global__ __launch_bounds__(256) void k_plane_transpose(const float *plane, float *out, int w0, int h0)
{
    __shared__ float t[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    int x = blockIdx.x * 16 + tx, y = blockIdx.y * 16 + ty;
    if (x < w0 && y < h0) t[ty][tx] = plane[(size_t) y * w0 + x];
    __syncthreads();
    x = blockIdx.x * 16 + ty; y = blockIdx.y * 16 + tx;
    if (x < w0 && y < h0) out[(size_t) x * h0 + y] = t[tx][ty];
}
