// Host twin of the raw-limb cases of bbgpu_selftest_field (BBGPU_SELFTEST_WIDE_*): the same function the device self-test runs per lane
// (barretenberg_amd/csrc/selftest_raw.hpp over fe.hpp's C++ definition), in a host loop.  Test infrastructure: built and run by
// tests/test_gpu_wideq.py, which compares its output with the device's word for word.
//   fe_wideq_twin fq|fr <op> <in> <out>     in: m x 24 words (limbs of a, then of c, zeros) followed by m x 24 words (b, then d or e); out: m x 24 words
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/selftest_raw.hpp"

int main(int argc, char** argv)
{
    if (argc != 5 || (strcmp(argv[1], "fq") && strcmp(argv[1], "fr"))) return 2;
    const int op = atoi(argv[2]);
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % (2 * 24 * 4) != 0) return 2;
    const int m = (int)(bytes / (2 * 24 * 4));
    std::vector<uint32_t> in((size_t)m * 48), out((size_t)m * 24, 0u);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);
    const uint32_t *a = in.data(), *b = in.data() + (size_t)m * 24;
    for (int i = 0; i < m; i++) {
        if (argv[1][1] == 'q') bbgpu::raw_dispatch<bbgpu::FqP>(op, a, b, out.data(), m, i);
        else bbgpu::raw_dispatch<bbgpu::FrP>(op, a, b, out.data(), m, i);
    }
    f = fopen(argv[4], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
