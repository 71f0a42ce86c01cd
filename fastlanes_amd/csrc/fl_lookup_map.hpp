// fl_lookup_map.hpp -- the block routes and the tier of unfor_lookup (fl_lookup.hpp), shared by the kernel, the C ABI's host side and a
// CPU test that compiles this header with a plain C++ compiler (tests/test_lookup_cpu.py).  No HIP dependency.
//
// unfor_lookup is the PROBE side of a payload join over the dense window unfor_set_build, unfor_compare_in and
// unfor_aggregate_by_window share: a kept row with key k reads table[j], j = (k - key_lo) mod 2^T, when j < n_slots (and bit j of
// `present` is set, when a bitmap is given) and `missing` otherwise.  The window is unfor_compare_in's (fl_set_decide.hpp: set_window,
// set_block_decide), so a block is judged from its metadata and its mask before any packed byte is requested, by the probe side's rules:
//   SKIP      the block fails a device check: nothing is read, nothing is written, nothing is counted;
//   MISSING   the mask keeps nothing, or set_block_decide says SET_NONE -- no key of the block lies in the window: no packed byte and
//             no table byte is read, the whole output block is `missing`, no hit bit is set, every kept row counts as a miss;
//   ONE_SLOT  width 0 inside the window (SET_PROBE): every kept row has key = reference, so ONE wave-uniform table read (slot c) and
//             at most one `present` bit answer the block, broadcast under the mask;
//   EACH      everything else is decoded and gathered.
#pragma once
#include "fl_set_decide.hpp"

namespace fl {

enum LookupRoute { LOOKUP_SKIP = 0, LOOKUP_MISSING = 1, LOOKUP_ONE_SLOT = 2, LOOKUP_EACH = 3 };
enum LookupTier { LOOKUP_LDS = 0, LOOKUP_MEM = 1 };

// Up to this many bytes a wavefront keeps a PRIVATE copy of the table in LDS: the bytes unfor_set_build's private bitmap takes
// (SET_BUILD_LDS_BITS / 8), so the LDS tier's footprint per wavefront is that of a shipped kernel.  A larger table is gathered from
// device memory through one bounded buffer descriptor.
constexpr uint64_t LOOKUP_LDS_BYTES = 8192;
// the descriptor's offsets are 32-bit with the top bit free for "outside": a table must stay below this many bytes
constexpr uint64_t LOOKUP_MAX_TABLE_BYTES = 1ull << 31;

// the route of a block and c = (reference - key_lo) mod 2^T (ONE_SLOT: the slot, c <= window.s; EACH: the summand of every field)
FL_HD inline LookupRoute lookup_route(unsigned type_bits, const ForPredicate& window, bool mask_empty, bool precondition_ok, uint64_t reference,
                                      unsigned width, uint64_t& c)
{
    c = (reference - window.a) & type_max(type_bits);
    if (!precondition_ok) return LOOKUP_SKIP;
    if (mask_empty) return LOOKUP_MISSING;
    const int v = set_block_decide(type_bits, window, reference, width, c);
    return v == SET_NONE ? LOOKUP_MISSING : v == SET_PROBE ? LOOKUP_ONE_SLOT : LOOKUP_EACH;
}
// whether the route requests packed bytes (a width-0 block never does: it is MISSING or ONE_SLOT) / reads the table at all
FL_HD inline bool lookup_reads_packed(LookupRoute route) { return route == LOOKUP_EACH; }
FL_HD inline bool lookup_reads_table(LookupRoute route) { return route == LOOKUP_ONE_SLOT || route == LOOKUP_EACH; }
// whether the route writes the block's output (every valid block's output block is always written)
FL_HD inline bool lookup_writes_block(LookupRoute route) { return route != LOOKUP_SKIP; }

// what a block decided WITHOUT a gather adds to stats[1] (misses), given the rows its mask keeps (ONE_SLOT depends on the slot's bit)
FL_HD inline uint64_t lookup_decided_misses(LookupRoute route, uint64_t kept) { return route == LOOKUP_MISSING ? kept : 0; }

// n_slots the entry points refuse (FL_ERR_INDEX): above min(2^T, 2^32) slots, or a table of 2^31 bytes or more
FL_HD inline bool lookup_slots_refused(unsigned type_bits, uint64_t n_slots, unsigned payload_bytes)
{
    return n_slots > set_max_bits(type_bits) || n_slots * payload_bytes >= LOOKUP_MAX_TABLE_BYTES;
}

// the tier of a call, chosen once on the host: the table's bytes against the private copy's
FL_HD inline LookupTier lookup_tier(uint64_t n_slots, unsigned payload_bytes)
{
    return n_slots * payload_bytes <= LOOKUP_LDS_BYTES ? LOOKUP_LDS : LOOKUP_MEM;
}

// the private table of the LDS tier: the largest table of the tier the key type can address (u8 keys: 256 slots)
FL_HD constexpr unsigned lookup_lds_table_bytes(unsigned type_bits, unsigned payload_bytes)
{
    return type_bits >= 16 ? (unsigned)LOOKUP_LDS_BYTES : (1u << type_bits) * payload_bytes;
}
// per-wavefront LDS: the block's image, then (LDS tier) the private table
FL_HD constexpr unsigned lookup_wave_lds(unsigned block_bytes, unsigned type_bits, unsigned payload_bytes, bool lds_tier)
{
    return block_bytes + (lds_tier ? lookup_lds_table_bytes(type_bits, payload_bytes) : 0u);
}

}  // namespace fl
