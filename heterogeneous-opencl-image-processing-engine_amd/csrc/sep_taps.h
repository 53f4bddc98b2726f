// sep_taps.h — internal: a validated separable kernel (mi_blur_sep_kernel, include/mi_blur.h) in the form the GPU
// kernels (sep_kernels.hip) and the CPU device (cpu_device.cpp) take it.  Plain C++, no HIP.
#pragma once

namespace mi_blur {

constexpr int SEP_MAX_R = 16;

// Taps CENTRED: wx[SEP_MAX_R + d] = weight of the pixel d columns away, 0 beyond the radius (likewise wy for rows),
// so loops unrolled over d index them with compile-time constants.
struct SepTaps {
    int rx, ry, shift;      // shift = bx + by: the one truncating shift at the end
    unsigned wx[2 * SEP_MAX_R + 1], wy[2 * SEP_MAX_R + 1];
};

}  // namespace mi_blur
