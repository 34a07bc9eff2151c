// Fast fused log-normalise + Gaussian blur instances for uint8_t input (blur_mfma.h, blur.h).
#include "blur_mfma.h"

namespace mw {
template int launch_blur_fast<uint8_t>(const uint8_t*, int, int, int, const float*, float, const BlurTaps&,
                                    int, float*, hipStream_t);
template int launch_blur_part<uint8_t>(const uint8_t*, int, int, int, const float*, float, const BlurTaps&, int,
                                     float*, const int*, int, hipStream_t);
}  // namespace mw
