// round2_dev.hpp — what the recruitment rounds of the device step share (round2.hip: round 1; round_n.hip: rounds 2 and later): the words
// of a round's statistics block, the (k-mer, gap) table's slot and its insert, the key layout gap << 40 | library << 36 | pair.
#pragma once
#include <algorithm>

#include "gf_internal.hpp"

namespace gf {

enum : uint32_t {
    R2_KMERS = 0,        // contig k-mer positions of the open gaps (the table's sizing count)
    R2_TAB_FULL = 1,     // (k-mer, gap) entries the table had no room for
    R2_HITS = 2,         // keys emitted by the recruitment (beyond the key capacity: not stored)
    R2_UNIQUE = 3,       // distinct (gap, library, pair)
    R2_TRIED = 4,        // gaps open after the first pick
    R2_WITH = 5,         // gaps with at least one recruited pair
    R2_ROWS = 6,         // u64 (words 6-7): rows of the round-2 pools
    R2_FIRST = 8,        // index of the first round-2 contig in the step's list
    R2_APPEND_ERR = 9,   // the round-2 contigs did not fit the step's list (nothing appended)
    R2_N2 = 10,          // round-2 contigs appended
    R2_POOL_OVF = 11,    // the round-2 pools did not fit their capacity (every round-2 pool left empty)
    R2_NEW = 12,         // rounds 2 and later: pairs new in this round, summed over the gaps open at its start
    R2_GROWN = 13,       // rounds 2 and later: gaps open at the round's start whose recruits grew
    R2_GATED = 14,       // rounds 2 and later: 1 when the round before grew no gap and this one did nothing
};

constexpr unsigned long long R2_EMPTY_KEY = ~0ull;

struct R2Slot {
    uint64_t hi, lo;
    uint32_t gap, state;
};
static_assert(sizeof(R2Slot) == 24, "slot layout");

struct LibRows {
    const uint8_t* reads[GF_R2_MAX_LIBS];
};

__device__ __forceinline__ bool r2_acgt(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

[[maybe_unused]] static __device__ void r2_insert(R2Slot* tab, uint32_t log2, K128 v, uint32_t gap, uint32_t* full) {
    const uint32_t mask = (uint32_t)((1ull << log2) - 1);
    uint32_t pos = hash_kmer(v, (int)log2);
    uint64_t probes = 0;
    while (probes <= mask) {
        R2Slot* s = tab + pos;
        const uint32_t st = __hip_atomic_load(&s->state, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (st == 0u) {
            if (atomicCAS(&s->state, 0u, 1u) == 0u) {
                __hip_atomic_store(&s->hi, v.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&s->lo, v.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&s->gap, gap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&s->state, 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            continue;            // lost the claim: read the same slot again
        }
        if (st == 1u) continue;  // being written: read it again in the next turn
        if (__hip_atomic_load(&s->hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == v.hi &&
            __hip_atomic_load(&s->lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == v.lo &&
            __hip_atomic_load(&s->gap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gap)
            return;              // (k-mer, gap) is in the table already
        pos = (pos + 1) & mask;
        ++probes;
    }
    atomicAdd(full, 1u);
}

__device__ __forceinline__ uint32_t key_gap(unsigned long long x) { return (uint32_t)(x >> 40); }

inline unsigned r2_grid(gf_ctx* ctx, uint64_t work) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->n_cu * 16, (work + 255) / 256));
}

}  // namespace gf
