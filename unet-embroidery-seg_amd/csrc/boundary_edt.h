// Limits and launcher of the exact squared Euclidean distance transform (boundary.hip), shared with the
// boundary loss (boundary_loss.hip), which runs it over both site maps of a batch in one call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kEdtInf = 1 << 30;  // UNETSEG_EDT_INF
constexpr int kEdtMax = 16384;    // largest H and W

// d2 int32 [N][H][W] = squared distance to the nearest non-zero pixel of the same image of sites uint8
// [N][H][W], kEdtInf without one; d2 is the only scratch.  Two or three launches on st, no host wait.  The
// caller has checked the arguments: N > 0, 0 < H, W <= kEdtMax.
void launch_edt_sqdist(const uint8_t* sites, int N, int H, int W, int32_t* d2, hipStream_t st);
