// The reference's MSM entry points, through the shim's mangled symbols, with the library bound to `contexts` device contexts on device 0
// (bbgpu_init_devices; 1 = the usual single context): a prover-shaped round of batched_scalar_multiplications over three 2^17-point jobs
// (prover.cpp:65-122 commits three polynomials at once), then pippenger() over the same table from four OpenMP threads at the same time.
// Prints every resulting point; tests/test_gpu_multi_context.py runs it with 1 and 2 contexts and compares the outputs byte for byte.
#include <omp.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/shim/bb_abi.hpp"
#include "../../include/bbgpu.h"

using namespace barretenberg;

static uint64_t sm_state;
static uint64_t splitmix()
{
    uint64_t z = (sm_state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

static void print_point(const char* what, int i, const g1::element& p)
{
    uint64_t w[12];
    std::memcpy(w, &p, sizeof(w));
    std::printf("%s %d", what, i);
    for (int k = 0; k < 12; k++) std::printf(" %016llx", (unsigned long long)w[k]);
    std::printf("\n");
}

int main(int argc, char** argv)
{
    const int contexts = argc > 1 ? atoi(argv[1]) : 1;
    const size_t n = (size_t)1 << 17;
    const int JOBS = 3, THREADS = 4;
    std::vector<int> devices((size_t)contexts, 0);
    if (bbgpu_init_devices(devices.data(), contexts) < 0) { // before the first shim call: the shim never binds by itself
        std::printf("FAIL init_devices: %s\n", bbgpu_last_error());
        return 1;
    }
    std::printf("contexts %d\n", bbgpu_num_contexts());
    sm_state = 7;
    uint64_t x[4] = { splitmix(), splitmix(), splitmix(), splitmix() & 0x0fffffffffffffffULL };
    g1::affine_element* table = static_cast<g1::affine_element*>(aligned_alloc(64, 2 * n * sizeof(g1::affine_element)));
    if (bbgpu_srs_generate(x, n, reinterpret_cast<uint64_t*>(table)) < 0) {
        std::printf("FAIL srs_generate: %s\n", bbgpu_last_error());
        return 1;
    }
    // a second copy of the table the library has never seen: registered on first sight (sliced over the contexts)
    g1::affine_element* fresh = static_cast<g1::affine_element*>(aligned_alloc(64, 2 * n * sizeof(g1::affine_element)));
    std::memcpy(fresh, table, 2 * n * sizeof(g1::affine_element));
    const int VEC = JOBS + THREADS;
    std::vector<fr::field_t*> sc((size_t)VEC);
    for (auto& s : sc) {
        s = static_cast<fr::field_t*>(aligned_alloc(32, n * sizeof(fr::field_t)));
        for (size_t i = 0; i < n; i++) {
            for (int l = 0; l < 4; l++) s[i].data[l] = splitmix();
            s[i].data[3] &= 0x1fffffffffffffffULL; // any representative below 2^253
        }
    }
    for (int round = 0; round < 2; round++) { // the second round finds every slice resident
        scalar_multiplication::multiplication_state st[JOBS];
        for (int j = 0; j < JOBS; j++) {
            st[j].points = j == 1 ? fresh : table;
            st[j].scalars = sc[(size_t)j];
            st[j].num_elements = n;
        }
        scalar_multiplication::batched_scalar_multiplications(st, JOBS);
        for (int j = 0; j < JOBS; j++) print_point("batch", j, st[j].output);
        std::vector<g1::element> part((size_t)THREADS);
        omp_set_num_threads(THREADS);
#pragma omp parallel for
        for (int t = 0; t < THREADS; t++)
            part[(size_t)t] = scalar_multiplication::pippenger(sc[(size_t)(JOBS + t)], (t & 1) ? fresh : table, n, 0);
        for (int t = 0; t < THREADS; t++) print_point("pippenger", t, part[(size_t)t]);
    }
    bbgpu_memory_info mi;
    for (int k = 0; k < contexts; k++)
        if (bbgpu_memory_stats_context(k, &mi) < 0) {
            std::printf("FAIL memory_stats_context %d\n", k);
            return 1;
        }
    bbgpu_shutdown();
    for (auto* s : sc) free(s);
    free(fresh);
    free(table);
    std::printf("DONE\n");
    return 0;
}
