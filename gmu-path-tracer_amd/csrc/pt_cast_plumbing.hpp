// The persistent-wave plumbing of the two fused ray casts, k_cast_w (pt_traverse_wide.hip, the default) and k_cast_f (pt_traverse.hip,
// cast0): everything around the walk.  The walks, the parking and the merge rules stay in the kernels.
//
// The protocol, once:
//   - CHUNKS.  A wave takes the queue entries of a phase (0: extension rays, 1: shadow rays) in chunks of p.raysPerWave <= 128 from the
//     device counter p.travCounters[phase]: one atomic per chunk, no wave waits for another.  A chunk lives in two registers per lane
//     (lane l holds entries l and 64 + l); a lane that needs a ray gets its entry from a neighbour's register by shuffle.  A claim beyond
//     the end of the queue moves the wave to the next phase; phase 2 is the drain.
//   - TAIL.  Towards the end of the LAST queue the chunks shrink, so that the waves run dry within half the time of each other: half
//     chunks once fewer than two rounds of the grid are left (the position is estimated from this wave's previous chunk: every other
//     wave has taken about one since), quarter chunks in the last half round where the caller asks for them.
//   - WHO MAY GIVE (drain only).  A lane with a ray that still walks and has deferred inner entries above `bottom`, up to twelve times
//     per ray; a helper gives parts of its subtree in turn.  A lane whose walk has ended never gives.  It gives the BOTTOM entry of its
//     stack: the subtree it would visit last, the largest one left.
//   - WHO MAY TAKE.  A lane without a ray.  The k-th free lane pairs with the k-th donor, all pairs of the wave at once; the taker
//     copies the donor's ray, walks the subtree on its own stack and records the donor's lane as its `owner`.
//   - WHEN AN OWNER IS WRITTEN BACK.  A helper that has finished (and has heard from its own helpers) reports owner, distance, hu, hv
//     and hitRef to its owner and becomes free; an owner's result is written only when its own walk has ended AND `outstanding` is back
//     at zero, how the reports merge being the kernel's rule.  Until then the lane is neither idle nor free.
//   - A wave that exceeds p.castLoopCap loop iterations has met a bug in this protocol: it flags the launch and leaves.
#pragma once
#include "pt_traverse_deferred.hpp"

namespace gmupt {

// Macros over the kernel's own names, not functions, wherever a function changes the shipped instruction streams (tools/isa_compare.py,
// profiles/cast_plumbing/): a loop-carried local kept in a struct or passed by reference, and even a small value function called between
// the ballots of the refill, is promoted to registers in another order and every instantiation's register allocation changes.

// The chunk of queue entries a wave is working through: entries [next, end) are still to hand out, lastBase is where the previous chunk
// began, and the chunk sits in registers, lane l holding entries chunkBase + l (qe0) and chunkBase + 64 + l (qe1).
#define GMUPT_CHUNK_CURSOR \
    uint32_t next = 0, end = 0, lastBase = 0; \
    uint32_t chunkBase = 0, qe0 = kQueueHole, qe1 = kQueueHole;

// Claims the next chunk of the current phase, or advances the phase, until the cursor has entries or both queues are exhausted
// (wave-uniform).  Uses the kernel's cursor, phase, p, lane, countExt / countSh and qExt / qSh; the queue is read through ENTRY(q, i), two
// coalesced loads per chunk; QUARTER_TAIL: the last half round is handed out in quarter chunks.
#define GMUPT_CLAIM_CHUNK(ENTRY, QUARTER_TAIL) \
    while (next >= end && phase < 2) { \
        uint32_t base = 0; \
        const uint32_t count = phase == 0 ? countExt : countSh; \
        const uint32_t gridWaves = gridDim.x * (uint32_t)(kDefBlock / 64); \
        const bool tail = phase == 1 && lastBase + 2u * gridWaves * p.raysPerWave > count; \
        const bool tail2 = (QUARTER_TAIL) && phase == 1 && lastBase + gridWaves * p.raysPerWave / 2u > count; \
        const uint32_t req = tail2 ? (p.raysPerWave > 32u ? p.raysPerWave / 4u : p.raysPerWave) : tail ? (p.raysPerWave > 64u ? p.raysPerWave / 2u : p.raysPerWave) : p.raysPerWave; \
        if (lane == 0u) base = atomicAdd(&p.travCounters[phase], req); \
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base); \
        if (base < count) { \
            lastBase = base; chunkBase = base; \
            next = base; end = (base + req < count) ? base + req : count; \
            const uint32_t* q = phase == 0 ? qExt : qSh; \
            qe0 = (base + lane < end) ? ENTRY(q, base + lane) : kQueueHole; \
            qe1 = (base + 64u + lane < end) ? ENTRY(q, base + 64u + lane) : kQueueHole; \
        } else { phase++; next = end = 0; lastBase = 0; } \
    }
#define GMUPT_PLAIN_ENTRY(Q, I) (Q)[I]   // a queue in memory, read as it is (k_cast_f)

// The queue entry for this idle lane (extensionRayCast.hlsl:210 / shadowRayCast.hlsl:159), out of the chunk registers.  The shuffles are for
// EVERY lane of the wave (one that sat them out would not lend its registers); `take` and `newIndex` are for the idle lanes only.
#define GMUPT_CHUNK_SHUFFLE() \
    const uint32_t my = next + prefix_rank(idleMask); \
    const uint32_t entry = idle ? ((my - chunkBase) & 127u) : 0u; \
    const uint32_t entryLo = (uint32_t)__shfl((int)qe0, (int)(entry & 63u)), entryHi = (uint32_t)__shfl((int)qe1, (int)(entry & 63u));
#define GMUPT_CHUNK_ENTRY() \
    const bool take = my < end; \
    const uint32_t newIndex = take ? (entry < 64u ? entryLo : entryHi) : kQueueHole;
// after a refill: the idle lanes have taken their entries
#define GMUPT_CHUNK_ADVANCE() next = (next + (uint32_t)nIdle < end) ? next + (uint32_t)nIdle : end;

// The drain's pairing of donors (wantHelp) and free lanes.  In two steps, with what a donor takes off its stack between them in the
// kernel: drain_pair says who gives and who takes; GMUPT_DRAIN_SOURCE makes the donors post their lane number to lane k and the takers
// fetch it from there -- `src`, the donor of a taker, and SL, the lane to copy the ray from (the lane's own for everybody else).
struct DrainPair { bool gives, takes; uint32_t dRank, fRank; };
__device__ __forceinline__ DrainPair drain_pair(unsigned long long wantHelp, unsigned long long freeLanes, uint32_t lane, bool haveRay)
{
    const uint32_t nDonors = (uint32_t)__popcll(wantHelp), nFree = (uint32_t)__popcll(freeLanes);
    const uint32_t nPairs = nDonors < nFree ? nDonors : nFree;
    const bool isDonor = ((wantHelp >> lane) & 1ull) != 0ull;
    DrainPair r;
    r.dRank = prefix_rank(wantHelp); r.fRank = prefix_rank(freeLanes);
    r.gives = isDonor && r.dRank < nPairs; r.takes = !haveRay && r.fRank < nPairs;
    return r;
}
#define GMUPT_DRAIN_SOURCE(PR, SL) \
    const int donorOfRank = __builtin_amdgcn_ds_permute((int)(((PR).gives ? (PR).dRank : 63u) << 2), (PR).gives ? (int)lane : 0); \
    const int src = __shfl(donorOfRank, (PR).takes ? (int)(PR).fRank : 0); \
    const int SL = (PR).takes ? src : (int)lane;

// What a finished helper (lane hl) tells the wave: ol (its owner's lane) and th, uh, vh, rh (its distance, hu, hv and hitRef)
#define GMUPT_HELPER_REPORT() \
    const int ol = __builtin_amdgcn_readlane(owner, hl); \
    const float th = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, distance), hl)); \
    const float uh = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hu), hl)); \
    const float vh = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hv), hl)); \
    const int rh = __builtin_amdgcn_readlane(hitRef, hl);

// Watchdog: a persistent kernel must end whatever happens.  A wave of the bench scene runs ~150 loop iterations per launch, one of the 10 M-
// triangle scene ~600; at the limit (2^20 by default; GMUPT_CAST_LOOP_CAP) it flags the launch (GMUPT_STAT_CAST_ABORTED: results invalid) and leaves.
#define GMUPT_WATCHDOG() if (++loopCount > p.castLoopCap) { if (lane == 0u) atomicOr(&p.stats->stackOverflow, 2u); break; }

// ---- the STATS epilogue of a wave (collect_stats builds of the kernels only)
__device__ __forceinline__ void flush_cast_counts(DevStats* st, const TravCount& tcE, uint32_t raysE, uint32_t wInE, uint32_t wTrE, const TravCount& tcS, uint32_t raysS,
                                                  uint32_t wInS, uint32_t wTrS, uint32_t topE, uint32_t topS, uint32_t helped, uint32_t nested)
{
    flush_counts(st, tcE, raysE, true); flush_wave_iters(st, wInE, wTrE, true);
    flush_counts(st, tcS, raysS, false); flush_wave_iters(st, wInS, wTrS, false);
    flush_sum(&st->extTopInner, topE); flush_sum(&st->shTopInner, topS); flush_sum(&st->castHelperSubtrees, helped); flush_sum(&st->castNestedHelpers, nested);
}
// lane 0 at the wave's exit (100 MHz ticks): the share of the drain, then the wave's lifetime and the lane census.  The wave counts itself
// (castWaves) in the kernel: the two kernels do so at different points of this sequence, and the order of the atomics is part of their streams.
__device__ __forceinline__ void flush_drain_share(DevStats* st, unsigned long long tEnd, unsigned long long tDrain, uint32_t drainIters, uint32_t drainBusy)
{
    atomicAdd(&st->castDrainClocks, tDrain ? tEnd - tDrain : 0ull); atomicAdd(&st->castDrainIters, (unsigned long long)drainIters);
    atomicAdd(&st->castDrainBusyLanes, (unsigned long long)drainBusy);
}
__device__ __forceinline__ void flush_wave_life(DevStats* st, unsigned long long life, uint32_t census0, uint32_t census1, uint32_t census2, uint32_t census3)
{
    atomicAdd(&st->castWaveClocks, life); atomicMax(&st->castWaveClocksMax, life);
    atomicAdd(&st->castWaveEndHist[life / 5000ull < 31ull ? life / 5000ull : 31ull], 1ull);
    atomicAdd(&st->laneCensus[0], (unsigned long long)census0); atomicAdd(&st->laneCensus[1], (unsigned long long)census1);
    atomicAdd(&st->laneCensus[2], (unsigned long long)census2); atomicAdd(&st->laneCensus[3], (unsigned long long)census3);
}

} // namespace gmupt
