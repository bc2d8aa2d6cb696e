// ae_codes.hpp -- binary codes of the two-mode latent prior (vaeb_ae_encode_bits /
// vaeb_ae_decode_bits, include/vaeb_hip.h): the posterior mean truncated to its nearer mode.
//   pack     bit j of row m = mu[m][j] >= a / 2, into words [M][ceil(Dz / 32)]: bit j at word
//            j / 32, bit j % 32; the padding bits of a row's last word are 0
//   unpack   z[m][j] = a where the bit is set, else 0: the rows the decoder is fed
// One thread per word (pack) or per element (unpack); each writes its own output only.
#pragma once
#include <cstdint>

namespace vaeb {
namespace ae {

__global__ __launch_bounds__(256) void ae_pack_bits_kernel(const float* mu, int M, int Dz, float half_a, uint32_t* words) {
    const int nw = (Dz + 31) / 32;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)M * nw) return;
    const int m = (int)(i / nw), w = (int)(i - (int64_t)m * nw);
    const float* row = mu + (int64_t)m * Dz;
    const int j1 = min(Dz, 32 * w + 32);
    uint32_t bits = 0u;
    for (int j = 32 * w; j < j1; ++j) bits |= (row[j] >= half_a ? 1u : 0u) << (j & 31);
    words[i] = bits;
}

__global__ __launch_bounds__(256) void ae_unpack_bits_kernel(const uint32_t* words, int M, int Dz, float a, float* z) {
    const int nw = (Dz + 31) / 32;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)M * Dz) return;
    const int m = (int)(i / Dz), j = (int)(i - (int64_t)m * Dz);
    z[i] = (words[(int64_t)m * nw + (j >> 5)] >> (j & 31)) & 1u ? a : 0.f;
}

}  // namespace ae
}  // namespace vaeb
