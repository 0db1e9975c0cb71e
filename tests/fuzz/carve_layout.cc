// Host check of csrc/carve.h (plain C++, built with the host sanitizers by tests/test_host_logic.py): sizes on the command line
// -> one line "off_0 ... off_k total"; every access a caller may make (size bytes from base + off) lands inside total() bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "carve.h"

int main(int argc, char **argv) {
    impop::Carve a, b;
    std::vector<size_t> size, off;
    for (int i = 1; i < argc; ++i) {
        size.push_back(strtoull(argv[i], nullptr, 10));
        off.push_back(i & 1 ? a.take_bytes(size.back()) : a.take<char>(size.back()));
        if (b.take_bytes(size.back()) != off.back()) return 1;  // the same sizes give the same layout
    }
    if (a.total() != b.total() || a.total() < a.used) return 1;
    std::vector<char> region(a.total() + 1, 0);  // the sanitizer sees any write past total() (+ 1: an empty layout has a base too)
    for (size_t k = 0; k < size.size(); ++k) {
        memset(impop::Carve::at<char>(region.data(), off[k]), (int)(k + 1), size[k]);
        printf("%zu ", off[k]);
    }
    for (size_t k = 0; k < size.size(); ++k)  // nobody wrote into anybody else's bytes
        for (size_t i = 0; i < size[k]; ++i)
            if (region[off[k] + i] != (char)(k + 1)) return 2;
    printf("%zu\n", a.total());
    return 0;
}
