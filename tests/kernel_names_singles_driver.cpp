// Prints the FOURTH list of ryg_rans_amd/csrc/kernel_names.hpp (RANS_AMD_KERNEL_NAMES_SINGLES), one `family<TAB>name<TAB>id` line
// per entry (tests/_batch_singles.py reads it).  g++ only: the header is host code.
#include <cstdio>
#include <cstring>

#include "kernel_names.hpp"

using namespace rans_amd;

int main()
{
    constexpr int kBefore = kKernelEntryCount + kAliasPairKernelEntryCount + kAliasPairEncodeKernelEntryCount;
    static_assert((int)kSinglesKernelEntries[0].id == kBefore + 1, "the fourth list's ids follow the third list's");
    static_assert((int)kAliasPairEncodeKernelEntries[0].id == kKernelEntryCount + kAliasPairKernelEntryCount + 1,
                  "the third list's ids are where they were");
    static_assert((int)kAliasPairKernelEntries[0].id == kKernelEntryCount + 1, "the second list's ids are where they were");
    static_assert((int)kKernelEntries[kKernelEntryCount - 1].id == kKernelEntryCount, "the first list's ids are where they were");
    static_assert(kKernelEntryCount == 53 && kAliasPairKernelEntryCount == 1 && kAliasPairEncodeKernelEntryCount == 1,
                  "the first three lists hold what they held");
    int row = 0;
    for (const KernelEntry &e : kSinglesKernelEntries) {
        if ((int)e.id != kBefore + 1 + row++)
            return 3; // (an id is not its row's place behind the first three lists)
        if (strcmp(kernel_name(e.id), e.name) != 0 || kernel_family(e.id) != e.family || kernel_entry(e.id).id != e.id)
            return 1; // (an id does not lead back to its own row)
        for (const KernelEntry &f : kKernelEntries)
            if (strcmp(f.name, e.name) == 0 || strcmp(f.family_name, e.family_name) == 0)
                return 2; // (a name or a family of the first list)
        for (const KernelEntry &f : kAliasPairKernelEntries)
            if (strcmp(f.name, e.name) == 0 || strcmp(f.family_name, e.family_name) == 0)
                return 2; // (... or of the second)
        for (const KernelEntry &f : kAliasPairEncodeKernelEntries)
            if (strcmp(f.name, e.name) == 0 || strcmp(f.family_name, e.family_name) == 0)
                return 2; // (... or of the third)
        printf("%s\t%s\t%d\n", e.family_name, e.name, (int)e.id);
    }
    return 0;
}
