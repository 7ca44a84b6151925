// Prints the registry of ryg_rans_amd/csrc/kernel_names.hpp, one `family<TAB>name` line per entry (tests/_kernel_rows.py reads
// it).  g++ only: the header is host code.
#include <cstdio>
#include <cstring>

#include "kernel_names.hpp"

using namespace rans_amd;

int main()
{
    static_assert(kernel_name(KernelId::none)[0] == '\0', "no launch has no name");
    for (const KernelEntry &e : kKernelEntries) {
        if (strcmp(kernel_name(e.id), e.name) != 0 || kernel_family(e.id) != e.family)
            return 1; // (an id does not lead back to its own row)
        printf("%s\t%s\n", e.family_name, e.name);
    }
    return 0;
}
