// zklaim_public.hip.hpp — the verifier's view of a zklaim payload and the bit rule that turns it into public inputs, for the host and the
// device alike (k_zklaim_input_sums in verify.hip, zkg_zklaim_input_map_mirror in setup_verify.hip).
//
// zklaim_input_map (zkg_zklaim_input_map, zklaim_circuit.hip) strings together, per payload, 32 hash bytes, 64 reference bytes (five
// little-endian u64, three zero slots) and 64 op bytes (a one-hot byte per 8-byte slot), reads every byte most significant bit first, and
// packs bit b of the whole string into element b / 253 with weight 2^(b mod 253).  With every byte bit-reversed the string is one
// little-endian integer and element k is its bits [253 k, 253 k + 253): eight words cut out of 33 bytes.
//
// Record of one payload as it is uploaded, ZV_REC = 80 bytes (the 160-byte string without its constant zeros):
//    0 .. 31   hash
//   32 .. 71   data_ref[0 .. 4], little-endian u64 (the string's bytes 32 .. 71: same offsets)
//   72 .. 76   per op slot: 1 + the index of the byte set_ops sets in that slot (less 1, less_or_eq 2, eq 3, greater_or_eq 4, greater 5,
//              not_eq 6, noop 7), 0 for any other enum value (set_ops' default: no byte set)
//   77 .. 79   zero
#pragma once
#include "fp.hip.hpp"

namespace zk {

static constexpr uint32_t ZV_REC = 80, ZV_STRING_BYTES = 160, ZV_FR_CAPACITY = 253;
// public inputs of a credential with npl payloads
ZK_HD uint32_t zv_input_count(uint32_t npl) { return (ZV_STRING_BYTES * 8 * npl + ZV_FR_CAPACITY - 1) / ZV_FR_CAPACITY; }

// byte B of the string of npl payloads, its bits reversed; zero behind the end
ZK_HD uint32_t zv_string_byte(const uint8_t *rec, uint32_t npl, uint32_t B) {
    if (B >= ZV_STRING_BYTES * npl) return 0;
    const uint8_t *r = rec + (size_t)(B / ZV_STRING_BYTES) * ZV_REC;
    const uint32_t i = B % ZV_STRING_BYTES;
    uint32_t v = 0;
    if (i < 72) v = r[i];                                                   // hash, reference values
    else if (i >= 96 && i < 136) v = r[72 + ((i - 96) >> 3)] == ((i - 96) & 7u) + 1u ? 1u : 0u;      // the five op slots
    v = ((v & 0xF0u) >> 4) | ((v & 0x0Fu) << 4);
    v = ((v & 0xCCu) >> 2) | ((v & 0x33u) << 2);
    return ((v & 0xAAu) >> 1) | ((v & 0x55u) << 1);
}

// element k of the input map: its value (below 2^253 < r) as eight little-endian words, NOT in Montgomery form
ZK_HD void zv_input_element(const uint8_t *rec, uint32_t npl, uint32_t k, uint32_t out[8]) {
    const uint32_t b0 = ZV_FR_CAPACITY * k, o = b0 >> 3, sh = b0 & 7u;
    uint32_t last = zv_string_byte(rec, npl, o);
#pragma unroll
    for (uint32_t w = 0; w < 8; ++w) {
        uint64_t acc = last;
#pragma unroll
        for (uint32_t j = 1; j <= 4; ++j) { last = zv_string_byte(rec, npl, o + 4 * w + j); acc |= (uint64_t)last << (8 * j); }
        out[w] = (uint32_t)(acc >> sh);
    }
    out[7] &= (1u << (ZV_FR_CAPACITY - 224)) - 1u;
}

}  // namespace zk
