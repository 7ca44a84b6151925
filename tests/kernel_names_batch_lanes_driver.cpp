// Prints the SECOND list of ryg_rans_amd/csrc/kernel_names.hpp (RANS_AMD_KERNEL_NAMES_LANES), one `family<TAB>name` line per
// entry (tests/_batch_lanes.py reads it).  g++ only: the header is host code.
#include <cstdio>
#include <cstring>

#include "kernel_names.hpp"

using namespace rans_amd;

int main()
{
    static_assert(kernel_name(KernelId::none)[0] == '\0', "no launch has no name");
    static_assert((int)kLaneKernelEntries[0].id == kKernelEntryCount + 1, "the second list's ids follow the first list's");
    for (const KernelEntry &e : kLaneKernelEntries) {
        if (strcmp(kernel_name(e.id), e.name) != 0 || kernel_family(e.id) != e.family)
            return 1; // (an id does not lead back to its own row)
        for (const KernelEntry &f : kKernelEntries)
            if (strcmp(f.name, e.name) == 0)
                return 2; // (a name of the first list)
        printf("%s\t%s\n", e.family_name, e.name);
    }
    return 0;
}
