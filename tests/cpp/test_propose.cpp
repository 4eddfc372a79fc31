// test_propose.cpp -- bf::ModelProposer::propose_from_best (host/better_flow/model_proposer.h) on arrays read from a file, its
// results written as raw bytes for tests/test_propose_cpu.py to compare with the numpy restatement.  Links nothing but libm and
// libstdc++: the device entry stays an unresolved weak symbol.
//
//   test_propose <in.bin> <out_prefix>
// in.bin: int64 n; the 7 doubles of bf_global_search_opts; the 8 int32 of bf_propose_opts; max_score[n], best_nx[n],
// best_ny[n] as doubles.  Writes <prefix>proposals.bin, models.bin, info.bin, H.u32, B.u32.
#include <better_flow/model_proposer.h>

#include <cstdio>
#include <string>

static bool write_all(const std::string &path, const void *p, size_t bytes) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: test_propose <in.bin> <out_prefix>\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n = 0;
    bf_global_search_opts lattice;
    bf_propose_opts opts;
    static_assert(sizeof(lattice) == 7 * sizeof(double) && sizeof(opts) == 32, "layouts of the input file");
    bool ok = std::fread(&n, sizeof(n), 1, f) == 1 && std::fread(&lattice, sizeof(lattice), 1, f) == 1 &&
              std::fread(&opts, sizeof(opts), 1, f) == 1 && n >= 0;
    std::vector<double> ms, bx, by;
    if (ok) {
        ms.resize((size_t)n); bx.resize((size_t)n); by.resize((size_t)n);
        for (std::vector<double> *a : {&ms, &bx, &by}) ok = ok && (n == 0 || std::fread(a->data(), sizeof(double), (size_t)n, f) == (size_t)n);
    }
    std::fclose(f);
    if (!ok) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    std::printf("device entry %s\n", bf::ModelProposer::device_available() ? "linked" : "absent");
    bf::ModelProposer::Result r;
    const int rc = bf::ModelProposer::propose_from_best(bx.data(), by.data(), ms.data(), (size_t)n, lattice, opts, &r);
    std::printf("rc %d proposals %d\n", rc, (int)r.info.proposals);
    if (rc < 0) return 1;
    const std::string p = argv[2];
    ok = write_all(p + "proposals.bin", r.proposals.data(), r.proposals.size() * sizeof(bf_proposal)) &&
         write_all(p + "models.bin", r.models.data(), r.models.size() * sizeof(bf_model)) &&
         write_all(p + "info.bin", &r.info, sizeof(r.info)) && write_all(p + "H.u32", r.H.data(), r.H.size() * sizeof(uint32_t)) &&
         write_all(p + "B.u32", r.B.data(), r.B.size() * sizeof(uint32_t));
    return ok ? 0 : 1;
}
