// kernel_names.hpp -- the registry of the kernels a launcher can report (rans_amd_last_decode_kernel /
// rans_amd_last_encode_kernel).  Host-only and free of HIP: tests/kernel_names_driver.cpp prints it with g++.
//
// One row per kernel: identifier, the string the public getters return, family.  The launchers report a KernelId, so a name
// that is not in this table does not compile; the tests hold every row of a family to a row of expectations
// (tests/_kernel_rows.py).  The families:
//   uniform                   uniform chunks (rans_amd_decode / _encode* / _adaptive*)
//   batch                     ragged batches, one stream per wave
//   batch_models              ... with one model per stream
//   batch_word_groups_decode  ragged 8-way word streams, eight per wave, decoder (RANS_AMD_OPT_BATCH_GROUPS)
//   batch_word_groups_encode  ... encoder (RANS_AMD_OPT_BATCH_ENCODE_GROUPS)
//   batch_byte_pairs_decode   ragged 2-way byte streams, 32 per wave, decoder (RANS_AMD_OPT_BATCH_PAIRS)
//   batch_byte_pairs_encode   ... encoder (RANS_AMD_OPT_BATCH_ENCODE_PAIRS)
//   batch_r64_lanes_decode    ragged 2-way rans64 streams, 64 per wave, decoder (RANS_AMD_OPT_BATCH_LANES)
//   batch_r64_lanes_encode    ... encoder (RANS_AMD_OPT_BATCH_ENCODE_LANES)
// A second list follows the first one: RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS, the family
//   batch_alias_pairs_decode  ragged 2-way alias streams, 32 per wave, decoder (RANS_AMD_OPT_BATCH_ALIAS_PAIRS)
// Its ids follow the first list's in KernelId, its rows are kAliasPairKernelEntries; kKernelEntries (what
// tests/kernel_names_driver.cpp prints and tests/_kernel_rows.py reads) is the first list alone, and
// tests/kernel_names_alias_pairs_driver.cpp with tests/_batch_alias_pairs.py hold the second list to its rows.
// A third list follows the second: RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS_ENCODE, the family
//   batch_alias_pairs_encode  ... encoder (RANS_AMD_OPT_BATCH_ENCODE_ALIAS_PAIRS)
// Its ids follow the second list's, its rows are kAliasPairEncodeKernelEntries; tests/kernel_names_alias_pairs_encode_driver.cpp
// with tests/_batch_encode_alias_pairs.py hold it to its rows.
// A fourth list follows the third: RANS_AMD_KERNEL_NAMES_SINGLES, the family
//   batch_singles_decode      ragged 1-way streams of all four formats, 64 per wave, decoder (RANS_AMD_OPT_BATCH_SINGLES)
// Its ids follow the third list's (56..59), its rows are kSinglesKernelEntries; tests/kernel_names_singles_driver.cpp with
// tests/_batch_singles.py hold it to its rows.
// kernel_entry(), kernel_name() and kernel_family() resolve ids from all four.  (Folding the lists into one is a later refactor:
// the row module has to know the families first, and the printed lines and counts of the first two lists are pinned by tests.)
// Nine families in the first list: a new kernel is one more row at the list's end (an id is its row's place, counted from 1, and the
// ids that exist stay where they are); tests/kernel_names_driver.cpp prints every row and tests/_kernel_rows.py reads them.
#pragma once

namespace rans_amd {

#define RANS_AMD_KERNEL_NAMES(X)                                                                  \
    X(decode_word64, "k_decode_word64", uniform)                                                  \
    X(decode_word, "k_decode<word>", uniform)                                                     \
    X(decode_word_u16, "k_decode<word, u16 symbols>", uniform)                                    \
    X(decode_word_chunk_models, "k_decode<word, per-chunk models>", uniform)                      \
    X(decode_byte, "k_decode<byte>", uniform)                                                     \
    X(decode_byte_slot_records, "k_decode<byte, slot records>", uniform)                          \
    X(decode_byte_chunk_models, "k_decode<byte, per-chunk models>", uniform)                      \
    X(decode_r64, "k_decode<r64>", uniform)                                                       \
    X(decode_r64_search, "k_decode<r64 search>", uniform)                                         \
    X(decode_alias, "k_decode<alias>", uniform)                                                   \
    X(decode_dual_alias, "k_decode_dual<alias>", uniform)                                         \
    X(decode_word_groups, "k_decode_word_groups", uniform)                                        \
    X(decode_byte_pairs, "k_decode_byte_pairs", uniform)                                          \
    X(decode_lanes, "k_decode_lanes", uniform)                                                    \
    X(decode_lanes_staged, "k_decode_lanes_staged", uniform)                                      \
    X(decode_lanes_r64x2, "k_decode_lanes_r64x2", uniform)                                        \
    X(decode_lanes_r64x2_packed, "k_decode_lanes_r64x2<packed slots>", uniform)                   \
    X(encode_word, "k_encode<word>", uniform)                                                     \
    X(encode_word_chunk_models, "k_encode<word, per-chunk models>", uniform)                      \
    X(encode_byte, "k_encode<byte>", uniform)                                                     \
    X(encode_byte_chunk_models, "k_encode<byte, per-chunk models>", uniform)                      \
    X(encode_r64, "k_encode<r64>", uniform)                                                       \
    X(encode_r64_full_width, "k_encode<r64 full-width>", uniform)                                 \
    X(encode_alias_lds_remap, "k_encode<alias, LDS remap>", uniform)                              \
    X(encode_adaptive_word, "k_encode_adaptive<word>", uniform)                                   \
    X(encode_adaptive_byte, "k_encode_adaptive<byte>", uniform)                                   \
    X(encode_word_groups, "k_encode_word_groups", uniform)                                        \
    X(encode_lanes16, "k_encode_lanes16", uniform)                                                \
    X(encode_lanes_staged, "k_encode_lanes_staged", uniform)                                      \
    X(encode_lanes_r64x2, "k_encode_lanes_r64x2", uniform)                                        \
    X(decode_batch_word64, "k_decode_batch_word64", batch)                                        \
    X(decode_batch_word, "k_decode_batch<word>", batch)                                           \
    X(decode_batch_word_u16, "k_decode_batch<word, u16 symbols>", batch)                          \
    X(decode_batch_byte, "k_decode_batch<byte>", batch)                                           \
    X(decode_batch_byte_slot_records, "k_decode_batch<byte, slot records>", batch)                \
    X(decode_batch_r64, "k_decode_batch<r64>", batch)                                             \
    X(decode_batch_r64_search, "k_decode_batch<r64 search>", batch)                               \
    X(decode_batch_alias, "k_decode_batch<alias>", batch)                                         \
    X(encode_batch_word, "k_encode_batch<word>", batch)                                           \
    X(encode_batch_byte, "k_encode_batch<byte>", batch)                                           \
    X(encode_batch_r64, "k_encode_batch<r64>", batch)                                             \
    X(encode_batch_r64_full_width, "k_encode_batch<r64 full-width>", batch)                       \
    X(encode_batch_alias_lds_remap, "k_encode_batch<alias, LDS remap>", batch)                    \
    X(decode_batch_models_word, "k_decode_batch_models<word>", batch_models)                      \
    X(decode_batch_models_byte, "k_decode_batch_models<byte>", batch_models)                      \
    X(encode_batch_models_word, "k_encode_batch_models<word>", batch_models)                      \
    X(encode_batch_models_byte, "k_encode_batch_models<byte>", batch_models)                      \
    X(decode_batch_word_groups, "k_decode_batch_word_groups", batch_word_groups_decode)           \
    X(encode_batch_word_groups, "k_encode_batch_word_groups", batch_word_groups_encode)           \
    X(decode_batch_byte_pairs, "k_decode_batch_byte_pairs", batch_byte_pairs_decode)              \
    X(encode_batch_byte_pairs, "k_encode_batch_byte_pairs", batch_byte_pairs_encode)              \
    X(decode_batch_r64_lanes, "k_decode_batch_r64_lanes", batch_r64_lanes_decode)                 \
    X(encode_batch_r64_lanes, "k_encode_batch_r64_lanes", batch_r64_lanes_encode)

#define RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS(X)                                                      \
    X(decode_batch_alias_pairs, "k_decode_batch_alias_pairs", batch_alias_pairs_decode)

#define RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS_ENCODE(X)                                               \
    X(encode_batch_alias_pairs, "k_encode_batch_alias_pairs", batch_alias_pairs_encode)

#define RANS_AMD_KERNEL_NAMES_SINGLES(X)                                                          \
    X(decode_batch_singles_byte, "k_decode_batch_singles<byte>", batch_singles_decode)            \
    X(decode_batch_singles_word, "k_decode_batch_singles<word>", batch_singles_decode)            \
    X(decode_batch_singles_r64, "k_decode_batch_singles<r64>", batch_singles_decode)              \
    X(decode_batch_singles_alias, "k_decode_batch_singles<alias>", batch_singles_decode)

enum class KernelFamily {
    uniform,
    batch,
    batch_models,
    batch_word_groups_decode,
    batch_word_groups_encode,
    batch_byte_pairs_decode,
    batch_byte_pairs_encode,
    batch_r64_lanes_decode,
    batch_r64_lanes_encode,
    batch_alias_pairs_decode,
    batch_alias_pairs_encode,
    batch_singles_decode,
};

enum class KernelId {
    none, // no launch yet: the name is ""
#define X(id, name, family) id,
    RANS_AMD_KERNEL_NAMES(X)
    RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS(X) // (behind the first list: an id of this one is kKernelEntryCount + 1 + its row)
    RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS_ENCODE(X) // (behind the second: kKernelEntryCount + kAliasPairKernelEntryCount + 1 + its row)
    RANS_AMD_KERNEL_NAMES_SINGLES(X) // (behind the third: ... + kAliasPairEncodeKernelEntryCount + 1 + its row)
#undef X
};

struct KernelEntry {
    KernelId id;
    const char *name;
    KernelFamily family;
    const char *family_name;
};

// every entry, in the table's order (KernelId::none is not one)
constexpr KernelEntry kKernelEntries[] = {
#define X(id, name, family) {KernelId::id, name, KernelFamily::family, #family},
    RANS_AMD_KERNEL_NAMES(X)
#undef X
};
constexpr int kKernelEntryCount = (int)(sizeof(kKernelEntries) / sizeof(kKernelEntries[0]));

// the second list's entries, in its order
constexpr KernelEntry kAliasPairKernelEntries[] = {
#define X(id, name, family) {KernelId::id, name, KernelFamily::family, #family},
    RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS(X)
#undef X
};
constexpr int kAliasPairKernelEntryCount = (int)(sizeof(kAliasPairKernelEntries) / sizeof(kAliasPairKernelEntries[0]));

// the third list's entries, in its order
constexpr KernelEntry kAliasPairEncodeKernelEntries[] = {
#define X(id, name, family) {KernelId::id, name, KernelFamily::family, #family},
    RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS_ENCODE(X)
#undef X
};
constexpr int kAliasPairEncodeKernelEntryCount = (int)(sizeof(kAliasPairEncodeKernelEntries) / sizeof(kAliasPairEncodeKernelEntries[0]));

// the fourth list's entries, in its order
constexpr KernelEntry kSinglesKernelEntries[] = {
#define X(id, name, family) {KernelId::id, name, KernelFamily::family, #family},
    RANS_AMD_KERNEL_NAMES_SINGLES(X)
#undef X
};
constexpr int kSinglesKernelEntryCount = (int)(sizeof(kSinglesKernelEntries) / sizeof(kSinglesKernelEntries[0]));

constexpr const KernelEntry &kernel_entry(KernelId id) // (not for KernelId::none)
{
    constexpr int second = kKernelEntryCount, third = second + kAliasPairKernelEntryCount, fourth = third + kAliasPairEncodeKernelEntryCount;
    return (int)id <= second   ? kKernelEntries[(int)id - 1]
           : (int)id <= third  ? kAliasPairKernelEntries[(int)id - 1 - second]
           : (int)id <= fourth ? kAliasPairEncodeKernelEntries[(int)id - 1 - third]
                               : kSinglesKernelEntries[(int)id - 1 - fourth];
}
constexpr const char *kernel_name(KernelId id) { return id == KernelId::none ? "" : kernel_entry(id).name; }
constexpr KernelFamily kernel_family(KernelId id) { return kernel_entry(id).family; } // (not for KernelId::none)
static_assert(kernel_entry(KernelId::encode_batch_r64_lanes).id == KernelId::encode_batch_r64_lanes &&
                  kernel_entry(KernelId::decode_batch_alias_pairs).id == KernelId::decode_batch_alias_pairs &&
                  kernel_entry(KernelId::encode_batch_alias_pairs).id == KernelId::encode_batch_alias_pairs &&
                  (int)KernelId::encode_batch_alias_pairs == 55 &&
                  kernel_entry(KernelId::decode_batch_singles_byte).id == KernelId::decode_batch_singles_byte &&
                  kernel_entry(KernelId::decode_batch_singles_alias).id == KernelId::decode_batch_singles_alias &&
                  (int)KernelId::decode_batch_singles_byte == 56 && (int)KernelId::decode_batch_singles_alias == 59,
              "ids of all four lists resolve to their own rows");

} // namespace rans_amd
