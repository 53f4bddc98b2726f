// kernel_common.h — internal (not part of the C ABI): what the seven kernel files (blur_kernels.hip, sep_kernels.hip,
// median_kernels.hip, morph_kernels.hip, bilateral_kernels.hip, conv_kernels.hip, layout_kernels.hip) share below launch(): the launch call, the blockIdx -> tile maps, the template
// dispatch, the argument checks and parameter fill every family repeats, and the host side of the direct layout.
// Everything here has internal linkage, so libmi_blur.so exports nothing from it.
#pragma once
#include "blur_launch.h"
#include "../../include/mi_blur.h"

#include <hip/hip_ext.h>
#include <limits.h>
#include <stdint.h>
#include <type_traits>

namespace mi_blur {

// ----------------------------------------------------------------------------------
// device side
// ----------------------------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// blockIdx -> tile.  Blocks b and b+8 share an XCD (round-robin dispatch); give each XCD a contiguous run of the
// n tiles so tile-edge halo rows are L2 hits.  A bijection of [0, n).  Speed only.
__device__ __forceinline__ unsigned xcd_contiguous(unsigned L, unsigned n)
{
    const unsigned q = n >> 3, r = n & 7u, x = L & 7u, k = L >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}
// The same idea at a finer grain: runs of `run` consecutive tiles (tiles that share halo rows: an image, a few tile rows)
// are dealt to the XCDs in turn, so an XCD's tiles still find their neighbours' rows in its own L2 while its stream walks
// the WHOLE buffer instead of one eighth of it.  A bijection of [0, n): the last n mod 8*run tiles map to themselves.
__device__ __forceinline__ unsigned xcd_runs(unsigned L, unsigned n, unsigned run)
{
    const unsigned span = 8u * run, full = n - n % span;
    if (L >= full) return L;
    const unsigned x = L & 7u, k = L >> 3, j = k / run, o = k - j * run;
    return (j * 8u + x) * run + o;
}
__device__ __forceinline__ unsigned xcd_map(unsigned L, unsigned n, int mode)
{
    return mode == 0 ? L : mode == 1 ? xcd_contiguous(L, n) : xcd_runs(L, n, (unsigned)mode);
}

// ----------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------
static inline int hip_status(hipError_t e) { return e == hipSuccess ? MI_BLUR_OK : MI_BLUR_ERR_HIP_BASE - (int)e; }

// One kernel launch.  On a LaunchDesc: the timestamped form exactly when the caller gave a start or stop event.
template <typename K, typename... A>
static int do_launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A &...args)
{
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return hip_status(hipGetLastError());
}
template <typename K, typename... A>
static int do_launch(K kernel, dim3 grid, dim3 block, size_t lds, const LaunchDesc &d, const A &...args)
{
    if (d.start || d.stop)
        hipExtLaunchKernelGGL(kernel, grid, block, lds, d.stream, d.start, d.stop, 0, args...);
    else
        hipLaunchKernelGGL(kernel, grid, block, lds, d.stream, args...);
    return hip_status(hipGetLastError());
}

// Runtime value -> template argument: dispatch<1, 2, 3, 4>(channels, [&](auto C) { return do_launch(kernel<C>, ...); })
// calls f with std::integral_constant<int, V> for the listed V that equals v and returns its status;
// MI_BLUR_ERR_INVALID when v is not listed.  Only the listed values are instantiated, in list order — which is the order
// of the kernels in the code object, so a list such as <16, 4, 8> keeps the order its `case` table had.
template <int... Vs, typename F>
static int dispatch(int v, F &&f)
{
    int status = MI_BLUR_ERR_INVALID;
    (void)(... || (v == Vs && (status = f(std::integral_constant<int, Vs>{}), true)));   // a left fold: instantiates in list order
    return status;
}

// The argument checks launch(), launch_sep(), launch_median(), launch_morph(), launch_bilateral() and launch_conv() share; every one of them is MI_BLUR_ERR_INVALID.
// What differs between the families (radius / taps, halo rows, strides, where n_images == 0 is answered) stays in them.
static inline int check_desc(const LaunchDesc &d, FilterKind kind)
{
    if (!d.filter || d.filter->kind != kind || !d.in || !d.out || d.in == d.out) return MI_BLUR_ERR_INVALID;
    if (d.width <= 0 || d.band_rows <= 0 || d.channels <= 0 || d.n_images < 0) return MI_BLUR_ERR_INVALID;
    if (d.y0 < 0 || d.y1 > d.band_rows || d.y0 >= d.y1) return MI_BLUR_ERR_INVALID;
    if ((long long)d.width * d.channels > INT_MAX / 2) return MI_BLUR_ERR_INVALID;
    if ((long long)d.width * d.channels * d.band_rows > INT_MAX) return MI_BLUR_ERR_INVALID;  // per-image 32-bit
    return MI_BLUR_OK;
}
// Dense sizes of one band and one output block, and whether a stride given is negative or smaller than that.
static inline long long dense_in(const LaunchDesc &d) { return (long long)d.band_rows * d.width * d.channels; }
static inline long long dense_out(const LaunchDesc &d) { return (long long)(d.y1 - d.y0) * d.width * d.channels; }
static inline bool strides_too_small(const LaunchDesc &d)
{
    return d.in_stride < 0 || d.out_stride < 0 || (d.in_stride && d.in_stride < dense_in(d)) || (d.out_stride && d.out_stride < dense_out(d));
}

// The members every kernel's parameter struct has under the same names (a template, not a base struct: the structs'
// names and layouts are the kernels' mangled names and kernarg layouts).  Stride 0 = laid end to end.
template <typename P>
static void fill_band(P &p, const LaunchDesc &d)
{
    p.in = d.in; p.out = d.out;
    p.pitch = d.width * d.channels; p.H = d.band_rows; p.y0 = d.y0;
    p.in_stride = d.in_stride ? d.in_stride : dense_in(d);
    p.out_stride = d.out_stride ? d.out_stride : dense_out(d);
}

// Grid of a byte-per-thread kernel: 256 threads per block, capped; the kernel grid-strides the rest.
static inline dim3 byte_grid(long long total)
{
    const long long blocks = (total + 255) / 256;
    return dim3((unsigned)(blocks > 256LL * 64 ? 256LL * 64 : blocks));
}

// The direct layout (blur_direct_kernel, blur_median_fast_kernel): lanes are consecutive 16-byte chunk columns of the
// flattened (image, band of bh rows, chunk column) space, 62 computing lanes per wave, 4 waves per block.  Its work is
// numbered in 32 bits: direct_fits() is that bound for the shortest band any of these kernels uses (4 rows).
static inline bool direct_fits(const LaunchDesc &d)
{
    const long long cpr = (long long)d.width * d.channels / 16, rows = d.y1 - d.y0;
    return (long long)d.n_images * ((rows + 3) / 4) * cpr < 0x7fffffffLL;
}
// Fills p.nbands, p.total and p.nblocks (p.cpr is set) and returns the grid.
template <typename P>
static dim3 direct_grid(P &p, const LaunchDesc &d, int bh)
{
    p.nbands = (d.y1 - d.y0 + bh - 1) / bh;
    p.total = (long long)d.n_images * p.nbands * p.cpr;
    const long long waves = (p.total + 61) / 62;
    p.nblocks = (unsigned)((waves + 3) / 4);
    return dim3(p.nblocks);
}

}  // namespace mi_blur
