// minimizer.hpp -- the order of the (w, k) minimizer rule (aim_hip.h, AIM_FEATURE_MINIMIZERS), shared by the index kernel (index.hpp),
// the seed kernel (seed.hpp) and the host build (capi_pipeline.hip).
//
// A valid k-mer of code c has the order key min_hash(c), the 32-bit finaliser of MurmurHash3: a bijection on 32 bits, so two k-mers tie
// only when they are the same k-mer, and min_unhash gives the code back -- the kernels keep one dword per position, the key, and
// recover the code of a selected position from it. An invalid k-mer compares greater than every valid key, 0xFFFFFFFF included.
// The one 32-bit value that hashes to 0xFFFFFFFF is 0x331DA083, which is no code: codes are below 4^14 = 2^28 (k <= 14 is checked at
// every entry point). So kMinInvalid = 0xFFFFFFFF is above every key a valid k-mer can have and a plain 32-bit compare is exact; the
// static_assert below is what has to be revisited, together with the compares, before k may pass 14.
#pragma once

#include <cstdint>

namespace aim {

constexpr uint32_t kMinInvalid = 0xFFFFFFFFu;
constexpr int kMinMaxK = 14;

constexpr uint32_t min_hash(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

constexpr uint32_t min_unhash(uint32_t x)   // min_unhash(min_hash(c)) == c
{
    x ^= x >> 16;
    x *= 0x7ed1b41du;                        // 0xc2b2ae35^-1 mod 2^32
    x ^= (x >> 13) ^ (x >> 26);
    x *= 0xa5cb9243u;                        // 0x85ebca6b^-1 mod 2^32
    x ^= x >> 16;
    return x;
}

static_assert(min_unhash(kMinInvalid) == 0x331DA083u && min_unhash(kMinInvalid) >= (1u << (2 * kMinMaxK)), "kMinInvalid must be no valid k-mer's key");
static_assert(min_unhash(min_hash(0x0ABCDEF1u)) == 0x0ABCDEF1u && min_hash(0) == 0, "min_unhash inverts min_hash");

}  // namespace aim
