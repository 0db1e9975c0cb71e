// Host driver for impop_sim_parse_many (csrc/simparse.hip compiled as C++) under a sanitizer: the files given on the command
// line, in both flavours and with 1, 3 and 16 worker threads, several rounds each; every per-file result must equal
// impop_sim_parse's.  Built twice by tests/test_sim_batch_host.py: -fsanitize=address,undefined and -fsanitize=thread.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "internal.h"

namespace impop {
static thread_local char g_err[1024];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
int hip_fail(hipError_t, const char *what, const char *, int) {
    set_error("hip: %s", what);
    return IMPOP_E_HIP;
}
}  // namespace impop

struct Snap {
    int rc = 0;
    uint32_t n = 0;
    uint64_t rows = 0, n_bad = 0;
    int64_t bad_line = -1;
    std::string names;
    std::vector<double> dense;
    std::vector<uint32_t> seen;
    bool operator==(const Snap &o) const {
        return rc == o.rc && n == o.n && rows == o.rows && n_bad == o.n_bad && bad_line == o.bad_line && names == o.names &&
               seen == o.seen && dense.size() == o.dense.size() &&
               (dense.empty() || memcmp(dense.data(), o.dense.data(), dense.size() * sizeof(double)) == 0);
    }
};

static Snap snap_of(int rc, impop_sim *h) {
    Snap s;
    s.rc = rc;
    if (rc != 0) return s;
    uint64_t nb = 0;
    impop_sim_info(h, &s.n, &s.rows, &nb, &s.bad_line, &s.n_bad);
    s.names.resize(nb ? nb : 1);
    impop_sim_names(h, &s.names[0]);
    s.dense.resize((size_t)s.n * s.n);
    impop_sim_dense(h, s.dense.data());
    s.seen.resize(s.n);
    impop_sim_first_seen(h, s.seen.data());
    return s;
}

int main(int argc, char **argv) {
    std::vector<const char *> paths;
    for (int i = 1; i < argc; ++i) paths.push_back(argv[i]);
    for (int rep = 0; rep < 3; ++rep)  // the same files several times: more work items than threads
        for (int i = 1; i < argc; ++i) paths.push_back(argv[i]);
    paths.push_back(nullptr);  // a NULL path is that entry's IMPOP_E_INVALID
    const uint64_t k = paths.size();
    uint64_t checked = 0, accepted = 0, declined = 0;
    for (int flavor = 0; flavor < 2; ++flavor) {
        std::vector<Snap> want(k);
        for (uint64_t i = 0; i < k; ++i) {
            impop_sim *h = nullptr;
            const int rc = paths[i] ? impop_sim_parse(paths[i], flavor, &h) : IMPOP_E_INVALID;
            want[i] = snap_of(rc, h);
            if (h) impop_sim_free(h);
        }
        for (int threads : {1, 3, 16})
            for (int round = 0; round < 4; ++round) {
                std::vector<impop_sim *> out(k, (impop_sim *)0x1);
                std::vector<int> rcs(k, 12345);
                if (impop_sim_parse_many(paths.data(), k, flavor, threads, out.data(), rcs.data()) != IMPOP_OK) return 2;
                for (uint64_t i = 0; i < k; ++i) {
                    if ((rcs[i] == 0) != (out[i] != nullptr)) return 3;
                    if (!(snap_of(rcs[i], out[i]) == want[i])) {
                        fprintf(stderr, "mismatch: file %s flavor %d threads %d\n", paths[i] ? paths[i] : "(null)", flavor, threads);
                        return 4;
                    }
                    if (out[i]) impop_sim_free(out[i]);
                    ++checked;
                    (rcs[i] == 0 ? accepted : declined)++;
                }
            }
    }
    printf("parse_many ok: %llu results, %llu accepted, %llu declined\n", (unsigned long long)checked, (unsigned long long)accepted,
           (unsigned long long)declined);
    return 0;
}
