// sam_reader_main.cpp -- runs the SAM parser of the host mirror (wepp_amd/host/sam_reader.cpp) on a file and prints
// the aligned reads, one per line: name <tab> 0-based start <tab> aligned string.  A refused input prints the error's
// message on stderr and exits with 2.  tests/test_sam_reader.py compares it with tests/sam_model.py, once built plain
// and once under AddressSanitizer + UBSan.
//   sam_reader_main FILE GENOME_SIZE MIN_PHRED
#include <cstdio>
#include <cstdlib>

#include "../../wepp_amd/host/sam_reader.hpp"

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: sam_reader_main FILE GENOME_SIZE MIN_PHRED\n"); return 1; }
    try {
        const size_t n = parse_sam(argv[1], (size_t)atoll(argv[2]), atoi(argv[3]), [](sam_aligned_read&& rd) {
            printf("%s\t%d\t%s\n", rd.raw_name.c_str(), rd.start_idx, rd.aligned_string.c_str());
        });
        fprintf(stderr, "%zu reads\n", n);
    } catch (const MAT::mat_error& e) {
        fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    return 0;
}
