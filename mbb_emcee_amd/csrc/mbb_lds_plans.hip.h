// mbb_lds_plans.hip.h -- the dynamic-LDS plans of the one-launch sampler kernels and of the served kernel (k_flowm,
// k_flowa, k_serve: mbb_flow.hip), and the constants they and the host share.  One definition for both sides: the
// kernel lays its LDS out by these, and the host launches it with the size they give (mbb_hip.hip).
#pragma once
#include <stddef.h>

#include "mbb_device.hip.h"
#include "mbb_flow_index.h"

// ---- k_flowm, sampler form 7 (mbb_flowm.hip.h)
constexpr int kFmProp = 16;    // doubles per hand-over record besides WalkerK: proposal 0..4, (dim-1) ln z,
                               // ln u, the two penalties, the walker's row as it is (9..13)
// dynamic LDS of a k_flowm launch besides the staged passband tables (bytes)
// (np = pairs of walkers a workgroup serves: the hand-over records and their control words are per pair;
// nunit: the quadrature's units, whose descriptors -- {slot, first chunk, end chunk, kind} and the four result
// slots of a tail unit's rows, 32 bytes a unit -- the Q waves read from LDS, not from global memory, inside a pass)
constexpr int kFmUnitBytes = 32;
__host__ __device__ constexpr size_t flowm_lds(size_t nb, size_t npart, bool cov_in_lds, size_t nunit, size_t np = 1)
{
    return np * kFmNB * sizeof(mbbd::WalkerK) +
           8 * (np * kFmNB * npart + 2 * nb + np * kFmNB * kFmProp + 2 * nb + (cov_in_lds ? nb * nb : 0)) +
           8 * (nb + 2) + 8 * (kFmNC * 64) + 128 * np + 32 + kFmUnitBytes * nunit;
}

// ---- k_flowa, sampler form 9 (mbb_flowa.hip.h)
constexpr int kFaMaxW = 8;      // walkers per workgroup and half
constexpr int kFaNB = 2;        // hand-over record buffers in LDS: half-step j uses buffer j mod kFaNB
constexpr int kFaRec = 10;      // doubles per proposal record besides WalkerK: proposal 0..4, (dim-1) ln z, ln u, the two penalties

// dynamic LDS of a k_flowa launch besides the staged passband tables (bytes)
__host__ __device__ constexpr size_t flowa_lds(size_t nb, size_t npart, bool cov_in_lds, size_t W)
{
    return kFaNB * W * (sizeof(mbbd::WalkerK) + 8 * npart + 8 * kFaRec) + 8 * W * nb + 8 * 2 * W * 8 + 16 * nb +
           (cov_in_lds ? 8 * nb * nb : 0) + 8 * (nb + 2) + 192 + 64;
}

// ---- k_serve, the served boundary (mbb_serve.hip.h)
constexpr unsigned long long kServeQuit = 0xffffull;           // the request's row count that means "leave"

// dynamic LDS of a k_serve launch besides the staged passband tables (bytes)
__host__ __device__ constexpr size_t serve_lds(size_t nb, size_t npart, bool cov_in_lds)
{
    return sizeof(mbbd::WalkerK) + 8 * npart + 8 * nb + 16 + 16 * nb + (cov_in_lds ? 8 * nb * nb : 0) + 8 * (nb + 2) + 64;
}
