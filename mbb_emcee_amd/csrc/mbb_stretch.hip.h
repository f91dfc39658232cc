// mbb_stretch.hip.h -- the random draw of the stretch move: Philox4x32-10, the proposal, and what a state row draws at a
// half-step.  On its own so that the test-only device probe (tests/_device_probe.hip) compiles exactly what the sampler
// kernels do (mbb_kernels.hip.h, mbb_flowm.hip.h, mbb_flowa.hip.h include it through mbb_kernels.hip.h).
#pragma once

// Philox4x32-10 (Salmon et al. 2011), counter = (row, 2 step + half), key = seed.
__device__ __forceinline__ void philox4x32(unsigned int c[4], unsigned int k0, unsigned int k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // one 32x32->64 multiply (v_mad_u64_u32) per product instead of a high and a low
        // half: integer multiplies are quarter rate and this sits on the latency path
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned int hi0 = (unsigned int)(p0 >> 32), lo0 = (unsigned int)p0;
        const unsigned int hi1 = (unsigned int)(p1 >> 32), lo1 = (unsigned int)p1;
        const unsigned int n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// The stretch move's proposal c - z (c - s), one rounding per coordinate wherever it is formed.
__device__ __forceinline__ double stretch_q(double cv, double sv, double zz)
{
    return __builtin_fma(-zz, cv - sv, cv);
}

// Philox draw of state row `row` at half-step (step, half): z of the stretch move, the
// partner's index in the other half, the uniform of the accept test.  The key (`seed`) carries the step's number in
// the sampler's LIFE, the counter the row and the half: what is drawn for a step does not depend on how a run was cut
// into launches -- run_mcmc(p0, 64) twice and run_mcmc(p0, 128) make the same chain (rounds 1-5 also counted the
// step's place in its launch, `step`: another grouping was another chain -- ADVICE r05).
__device__ __forceinline__ void stretch_draw(int row, int step, int half, unsigned long long seed,
                                             double stretch_a, int c_count, double &zz, int &pj, double &u3)
{
    (void)step;
    unsigned int c4[4] = {(unsigned int)row, (unsigned int)half, 0u, 0u};
    philox4x32(c4, (unsigned int)seed, (unsigned int)(seed >> 32));
    const double u1 = fma((double)(c4[0] >> 5), 67108864.0, (double)(c4[1] >> 6)) * (1.0 / 9007199254740992.0);   // (exact)
    const double u2 = (double)c4[2] * (1.0 / 4294967296.0);
    u3 = ((double)c4[3] + 0.5) * (1.0 / 4294967296.0);
    const double sq = fma(stretch_a - 1.0, u1, 1.0);
    zz = sq * sq / stretch_a;
    pj = (int)(u2 * (double)c_count);
    if (pj >= c_count) pj = c_count - 1;
}
