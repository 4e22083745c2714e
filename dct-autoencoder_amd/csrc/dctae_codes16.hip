// The int16-code instantiations of the encode's code sinks (dctae_sort_pack.h,
// include/dctae_codes16.h): a unit of their own, so the int64 kernels of
// dctae_kernels.hip compile exactly as they did alone.
#include "dctae_sort_pack.h"

namespace dctae {

void launch_sort_pack_c16(const ImgDesc* imgs, int n_img, int np2, const EncParams& ep, const TokenSinks& st,
                          const PackSinks& out, hipStream_t s, int kernel, int max_T) {
  launch_sort_pack_t<int16_t>(imgs, n_img, np2, ep, st, out, s, kernel, max_T);
}

void launch_pad_fill_c16(const int32_t* row_len, int n_rows, const EncParams& ep, uint8_t* key_pad,
                         const PackSinks& out, hipStream_t s) {
  launch_pad_fill_t<int16_t>(row_len, n_rows, ep, key_pad, out, s);
}

}  // namespace dctae
