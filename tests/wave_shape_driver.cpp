// Prints what ryg_rans_amd/csrc/wave_shape.hpp answers over its whole domain (tests/test_wave_shape.py reads it).
// g++ only: the header is host code.
#include <cstdio>

#include "wave_shape.hpp"

using namespace rans_amd;

int main()
{
    const struct { int fmt; const char *name; } fmts[] = {
        {FMT_WORD, "word"}, {FMT_BYTE, "byte"}, {FMT_BYTEF, "byte-fused"}, {FMT_R64, "r64"}, {FMT_R64S, "r64-search"},
        {FMT_WORD16, "word-u16"}, {FMT_BYTEA, "byte-adaptive"}, {FMT_WORDA, "word-adaptive"}, {FMT_ALIAS, "alias"}};
    for (unsigned n = 0; n <= 513; ++n)
        printf("K %u %d\n", n, wave_states_per_lane(n));
    for (const auto &f : fmts)
        for (unsigned n = 0; n <= 513; ++n)
            for (unsigned sb = 1; sb <= 2; ++sb)
                for (int aligned = 0; aligned < 2; ++aligned)
                    for (int ragged = 0; ragged < 2; ++ragged) {
                        const DecodeShape s = decode_shape(f.fmt, n, sb, aligned, ragged);
                        const char *out = s.out == OUT_SLOW ? "slow" : s.out == OUT_FAST8 ? "fast8" : s.out == OUT_FAST16 ? "fast16" : "?";
                        // the kernel the launcher's `if constexpr` chain instantiates for this answer, if any
                        const bool exists = s.K && (decode_is_word64(f.fmt, s.K, s.out) || decode_has(f.fmt, s.K, s.out, ragged));
                        printf("D %s %u %u %d %d %d %s %d %d\n", f.name, n, sb, aligned, ragged, s.K, out, (int)s.word64, (int)exists);
                    }
    for (const auto &f : fmts)
        for (unsigned addr = 0; addr < 8; ++addr)
            for (unsigned chunk = 4096; chunk <= 4099; ++chunk)
                printf("L %s %u %u %d\n", f.name, addr, chunk, (int)decode_out_aligned(f.fmt, addr, chunk));
    for (unsigned b = 0; b < 128; ++b) // bit 0 fused status .. bit 6 FMT_WORDA, in encode_mode's argument order
        printf("E %u %d\n", b, encode_mode(b & 1, b & 2, b & 4, b & 8, b & 16, b & 32, b & 64));
    const unsigned chunks[] = {4096, 5000, 8192, 16384, 32768};
    for (unsigned n = 0; n <= 513; ++n)
        for (unsigned chunk : chunks)
            for (unsigned b = 0; b < 8; ++b) {
                const AdaptShape s = adapt_shape(n, b & 1, b & 2, chunk, b & 4);
                printf("A %u %u %u %u %u %d %d\n", n, chunk, b & 1, (b >> 1) & 1, (b >> 2) & 1, s.K, s.RR);
            }
    return 0;
}
