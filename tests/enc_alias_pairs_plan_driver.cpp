// Prints the LDS plan of k_encode_batch_alias_pairs (ryg_rans_amd/csrc/pairs_plan.hpp enc_alias_pairs_plan), one
// `scale_bits<TAB>table_bytes<TAB>waves<TAB>lds_bytes<TAB>blocks_per_cu` line for scale_bits 0..17
// (tests/test_batch_encode_alias_pairs_host.py reads it).  g++ only: the header is host code.
#include <cstdio>

#include "pairs_plan.hpp"

using namespace rans_amd;

int main()
{
    static_assert(enc_alias_pairs_plan(16).waves == 13 && enc_alias_pairs_plan(14).blocks_per_cu == 2, "usable in constant expressions");
    for (unsigned sb = 0; sb <= 17; ++sb) {
        const EncAliasPairsPlan p = enc_alias_pairs_plan(sb);
        printf("%u\t%u\t%u\t%u\t%u\n", sb, p.table_bytes, p.waves, p.lds_bytes, p.blocks_per_cu);
    }
    return 0;
}
