// csrc/host_plonk_verify.hpp's verify_host_multi (host PRODUCT code: the host twin of bbgpu_plonk_verify_multi) compiled with
// -fsanitize=address,undefined and driven over tests/golden/plonk_verify.json (a data fixture: six circuits under one g2_x, honest and tampered proofs
// with the reference's verdicts; its path is argv[1]): ALL rows of all circuits as ONE batch, each under its own circuit's label, with the bisection;
// one circuit against verify_host; the same key twice with alternating labels.  A stand-alone program with its own main; built and run by
// tests/test_plonk_verify_multi_host.py::test_standalone_program_under_sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../barretenberg_amd/csrc/host_plonk_verify.hpp"

using namespace bbgpu::host;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); fails++; } } while (0)

static std::string read_file(const char* path)
{
    std::string text;
    FILE* f = fopen(path, "rb");
    if (!f) return text;
    char buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, k);
    fclose(f);
    return text;
}
// the string / number that follows "key": from `from` on
static size_t after_key(const std::string& t, const char* key, size_t from)
{
    const std::string k = std::string("\"") + key + "\":";
    const size_t at = t.find(k, from);
    return at == std::string::npos ? at : at + k.size();
}
static std::string string_at(const std::string& t, size_t at)
{
    const size_t a = t.find('"', at), b = t.find('"', a + 1);
    return t.substr(a + 1, b - a - 1);
}
// 64 hex digits, most significant first -> 4 words, least significant first
static void hex_field(const std::string& h, uint64_t out[4])
{
    for (int k = 0; k < 4; k++) out[k] = strtoull(h.substr(16 * (3 - k), 16).c_str(), nullptr, 16);
}

struct Row {
    std::string circuit, tamper;
    int status, verdict;
    uint64_t proof[BBGPU_PLONK_PROOF_WORDS];
};

int main(int argc, char** argv)
{
    const std::string t = read_file(argc > 1 ? argv[1] : "tests/golden/plonk_verify.json");
    CHECK(!t.empty(), "fixture not found");
    if (t.empty()) return 1;
    uint64_t g2_x[16];
    size_t at = after_key(t, "g2_x", 0);
    for (int i = 0; i < 16; i++) {
        const std::string h = string_at(t, at);
        g2_x[i] = strtoull(h.c_str(), nullptr, 16);
        at = t.find('"', t.find('"', at) + 1) + 1;
    }
    const char* names[6] = { "standard/32", "standard/1024", "bool/14", "mimc/30", "extended/32", "zerowire/32" };
    std::vector<VerifyKey> keys(6);
    for (int c = 0; c < 6; c++) {
        const size_t circ = after_key(t, names[c], 0);
        CHECK(circ != std::string::npos, "no circuit %s", names[c]);
        const size_t n = (size_t)atol(t.c_str() + after_key(t, "n", circ));
        const int widgets = atoi(t.c_str() + after_key(t, "widgets", circ));
        uint64_t vk[BBGPU_PLONK_VK_WORDS] = {};
        at = after_key(t, "vk", circ);
        for (int i = 0; i < 2 * verify_num_vk(widgets); i++) {
            hex_field(string_at(t, at), vk + 4 * i);
            at = t.find('"', t.find('"', at) + 1) + 1;
        }
        const char* why = "";
        CHECK(verify_key_init(&keys[c], n, widgets, vk, g2_x, &why) == BBGPU_OK, "key %s: %s", names[c], why);
    }
    std::vector<Row> rows;
    for (size_t r = after_key(t, "rows", 0); (r = after_key(t, "circuit", r)) != std::string::npos;) {
        Row row;
        row.circuit = string_at(t, r);
        row.tamper = string_at(t, after_key(t, "tamper", r));
        row.status = atoi(t.c_str() + after_key(t, "rule_status", r));
        row.verdict = atoi(t.c_str() + after_key(t, "reference_verdict", r));
        const std::string p = string_at(t, after_key(t, "proof", r));
        CHECK(p.size() == 16 * BBGPU_PLONK_PROOF_WORDS, "proof of %zu digits", p.size());
        for (int i = 0; i < BBGPU_PLONK_PROOF_WORDS; i++) row.proof[i] = strtoull(p.substr(16 * (size_t)i, 16).c_str(), nullptr, 16);
        rows.push_back(row);
    }
    CHECK(rows.size() >= 73, "%zu rows", rows.size());
    const uint64_t seed[4] = { 1, 2, 3, 4 };

    // all rows of all circuits as one batch, interleaved (row j, then row j + 37, ...) so that neighbours are of different circuits
    {
        std::vector<size_t> order;
        for (size_t j = 0; j < rows.size(); j++) order.push_back((j * 37) % rows.size());
        std::vector<uint64_t> batch(rows.size() * BBGPU_PLONK_PROOF_WORDS);
        std::vector<uint32_t> circuit(rows.size()), status(rows.size(), 99);
        uint64_t flagged = 0, first_flagged = UINT64_MAX, first_failing = UINT64_MAX;
        for (size_t j = 0; j < rows.size(); j++) {
            const Row& row = rows[order[j]];
            memcpy(&batch[j * BBGPU_PLONK_PROOF_WORDS], row.proof, sizeof row.proof);
            for (uint32_t c = 0; c < 6; c++)
                if (row.circuit == names[c]) circuit[j] = c;
            if (row.status && flagged++ == 0) first_flagged = j;
            if (!row.status && !row.verdict && first_failing == UINT64_MAX) first_failing = j;
        }
        bbgpu_plonk_verify_report R, R2;
        CHECK(verify_host_multi(keys.data(), keys.size(), g2_x, circuit.data(), batch.data(), rows.size(), seed, BBGPU_PLONK_VERIFY_LOCATE, status.data(), &R) == BBGPU_OK, "batch");
        for (size_t j = 0; j < rows.size(); j++) CHECK((int)status[j] == rows[order[j]].status, "batch: status[%zu] = %u", j, status[j]);
        CHECK(R.count == rows.size() && R.bad_status == flagged && R.first_bad_status == first_flagged, "batch: %llu flagged, first %llu",
              (unsigned long long)R.bad_status, (unsigned long long)R.first_bad_status);
        CHECK(R.pairing_checked == 1 && R.pairing_ok == 0 && R.first_bad_proof == first_failing, "batch: first bad proof %llu, want %llu",
              (unsigned long long)R.first_bad_proof, (unsigned long long)first_failing);
        CHECK(verify_host_multi(keys.data(), keys.size(), g2_x, circuit.data(), batch.data(), rows.size(), seed, BBGPU_PLONK_VERIFY_LOCATE, status.data(), &R2) == BBGPU_OK, "again");
        CHECK(!memcmp(&R, &R2, sizeof R), "one seed, two reports");
        // the rows the reference accepted, alone: one good batch of several circuits
        std::vector<uint64_t> good;
        std::vector<uint32_t> good_circuit;
        for (size_t j = 0; j < rows.size(); j++)
            if (rows[order[j]].verdict) {
                good.insert(good.end(), &batch[j * BBGPU_PLONK_PROOF_WORDS], &batch[(j + 1) * BBGPU_PLONK_PROOF_WORDS]);
                good_circuit.push_back(circuit[j]);
            }
        CHECK(verify_host_multi(keys.data(), keys.size(), g2_x, good_circuit.data(), good.data(), good_circuit.size(), seed, 0, status.data(), &R) == BBGPU_OK, "good");
        CHECK(R.bad_status == 0 && R.pairing_ok == 1 && good_circuit.size() >= 15, "the accepted rows: %zu, pairing_ok %u", good_circuit.size(), R.pairing_ok);
    }
    // one circuit: verify_host's report; the same key twice, labels alternating: its a, b and verdict
    {
        std::vector<uint64_t> batch;
        for (const Row& row : rows)
            if (row.circuit == "standard/32" && batch.size() < 12 * BBGPU_PLONK_PROOF_WORDS) batch.insert(batch.end(), row.proof, row.proof + BBGPU_PLONK_PROOF_WORDS);
        const size_t count = batch.size() / BBGPU_PLONK_PROOF_WORDS;
        std::vector<uint32_t> zeros(count, 0), alternating(count), s1(count), s2(count);
        for (size_t j = 0; j < count; j++) alternating[j] = (uint32_t)(j & 1);
        bbgpu_plonk_verify_report one, multi, twice;
        const std::vector<VerifyKey> same = { keys[0], keys[0] };
        CHECK(verify_host(keys[0], batch.data(), count, seed, BBGPU_PLONK_VERIFY_LOCATE, s1.data(), &one) == BBGPU_OK, "verify_host");
        CHECK(verify_host_multi(keys.data(), 1, g2_x, zeros.data(), batch.data(), count, seed, BBGPU_PLONK_VERIFY_LOCATE, s2.data(), &multi) == BBGPU_OK, "G = 1");
        CHECK(!memcmp(&one, &multi, sizeof one) && s1 == s2, "G = 1 is not verify_host's report");
        CHECK(verify_host_multi(same.data(), same.size(), g2_x, alternating.data(), batch.data(), count, seed, BBGPU_PLONK_VERIFY_LOCATE, s2.data(), &twice) == BBGPU_OK,
              "the same key twice");
        CHECK(!memcmp(&one, &twice, sizeof one) && s1 == s2, "the same key twice is not verify_host's report");
        CHECK(one.pairing_ok == 0 && one.first_bad_proof == 1, "first bad proof %llu", (unsigned long long)one.first_bad_proof);
    }
    printf(fails ? "%d failures\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
