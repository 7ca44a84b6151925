// Prints the THIRD list of ryg_rans_amd/csrc/kernel_names.hpp (RANS_AMD_KERNEL_NAMES_ALIAS_PAIRS_ENCODE), one `family<TAB>name`
// line per entry (tests/_batch_encode_alias_pairs.py reads it).  g++ only: the header is host code.
#include <cstdio>
#include <cstring>

#include "kernel_names.hpp"

using namespace rans_amd;

int main()
{
    static_assert((int)kAliasPairEncodeKernelEntries[0].id == kKernelEntryCount + kAliasPairKernelEntryCount + 1,
                  "the third list's ids follow the second list's");
    static_assert((int)kAliasPairKernelEntries[0].id == kKernelEntryCount + 1, "the second list's ids are where they were");
    static_assert((int)kKernelEntries[kKernelEntryCount - 1].id == kKernelEntryCount, "the first list's ids are where they were");
    int row = 0;
    for (const KernelEntry &e : kAliasPairEncodeKernelEntries) {
        if ((int)e.id != kKernelEntryCount + kAliasPairKernelEntryCount + 1 + row++)
            return 3; // (an id is not its row's place behind the first two lists)
        if (strcmp(kernel_name(e.id), e.name) != 0 || kernel_family(e.id) != e.family || kernel_entry(e.id).id != e.id)
            return 1; // (an id does not lead back to its own row)
        for (const KernelEntry &f : kKernelEntries)
            if (strcmp(f.name, e.name) == 0 || strcmp(f.family_name, e.family_name) == 0)
                return 2; // (a name or a family of the first list)
        for (const KernelEntry &f : kAliasPairKernelEntries)
            if (strcmp(f.name, e.name) == 0 || strcmp(f.family_name, e.family_name) == 0)
                return 2; // (... or of the second)
        printf("%s\t%s\n", e.family_name, e.name);
    }
    return 0;
}
