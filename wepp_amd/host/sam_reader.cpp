// sam_reader.cpp -- see sam_reader.hpp: sam::add_reads (src/WEPP/sam2pb.cpp:157-258) without the table.
#include "sam_reader.hpp"

#include <climits>

#include "pbwire.hpp"

using MAT::mat_error;

namespace {

// std::stoi as the reference uses it: an optional sign and leading digits, anything behind them ignored
int leading_int(std::string const& tok, const char* what, std::string const& where) {
    size_t i = 0;
    bool neg = false;
    if (i < tok.size() && (tok[i] == '+' || tok[i] == '-')) neg = tok[i++] == '-';
    if (i >= tok.size() || tok[i] < '0' || tok[i] > '9') throw mat_error(where + ": " + what + " '" + tok + "' is not a number");
    long long v = 0;
    for (; i < tok.size() && tok[i] >= '0' && tok[i] <= '9'; i++) {
        v = v * 10 + (tok[i] - '0');
        if (v > INT_MAX) throw mat_error(where + ": " + what + " '" + tok + "' is out of range");
    }
    return (int)(neg ? -v : v);
}

}  // namespace

bool parse_sam_line(std::string const& line, size_t lineno, int min_phred, sam_aligned_read& out) {
    const std::string where = "line " + std::to_string(lineno);
    std::vector<std::string> tokens;
    MAT::string_split(line, tokens);
    if (tokens.empty() || tokens[0][0] == '@') return false;
    if (tokens.size() < 11) throw mat_error(where + ": " + std::to_string(tokens.size()) + " fields, at least 11 expected");
    if (leading_int(tokens[1], "FLAG", where) & 4) return false;
    const int start_idx = leading_int(tokens[3], "POS", where);
    const std::string &cigar = tokens[5], &read_seq = tokens[9], &phred_seq = tokens[10];
    if (phred_seq == "*" || phred_seq.size() < read_seq.size()) throw mat_error(where + ": no base quality for every base of the query");

    // the chunks \d+[A-Za-z] of the CIGAR, found as the reference's regex finds them: a run of digits counts when a
    // letter follows it, everything else is passed over
    size_t seq_idx = 0;
    std::string build;
    for (size_t i = 0; i < cigar.size();) {
        if (cigar[i] < '0' || cigar[i] > '9') { i++; continue; }
        size_t j = i;
        long long len = 0;
        for (; j < cigar.size() && cigar[j] >= '0' && cigar[j] <= '9'; j++) {
            if (len <= 1000000000) len = len * 10 + (cigar[j] - '0');      // (saturates: refused below when it counts)
        }
        const bool letter = j < cigar.size() && ((cigar[j] >= 'A' && cigar[j] <= 'Z') || (cigar[j] >= 'a' && cigar[j] <= 'z'));
        if (!letter) { i = j; continue; }
        if (len > 1000000000) throw mat_error(where + ": CIGAR length in '" + cigar + "'");
        const char op = cigar[j];
        i = j + 1;
        const size_t n = (size_t)len;
        switch (op) {
        case 'I': seq_idx += n; break;                                  // (:201-208: the query moves, the aligned string does not)
        case 'D': build.append(n, '_'); break;                          // :210-216
        case 'N': build.append(n, 'N'); seq_idx += n; break;            // :218-224: the query index advances
        case 'H': break;                                                // :226-228
        case 'S': seq_idx += n; break;                                  // :230-234
        default:                                                        // :236-253
            for (size_t k = 0; k < n; k++, seq_idx++) {
                if (seq_idx >= read_seq.size()) throw mat_error(where + ": the CIGAR consumes more bases than the query holds");
                char alt = ((int)phred_seq[seq_idx] - 33) < min_phred ? 'N' : read_seq[seq_idx];
                if (alt != 'A' && alt != 'C' && alt != 'G' && alt != 'T' && alt != 'N') alt = 'N';
                build.push_back(alt);
            }
        }
    }
    if (build.empty()) throw mat_error(where + ": the CIGAR yields no aligned column");
    out.raw_name = std::move(tokens[0]);
    out.start_idx = start_idx - 1;
    out.aligned_string = std::move(build);
    return true;
}

size_t parse_sam(std::string const& filename, size_t genome_size, int min_phred, std::function<void(sam_aligned_read&&)> const& sink) {
    MAT::pbwire::Lines in(filename, "SAM");
    std::string line;
    size_t lineno = 0, n = 0;
    while (in.next(line)) {
        lineno++;
        sam_aligned_read rd;
        if (!parse_sam_line(line, lineno, min_phred, rd)) continue;
        if (rd.start_idx < 0 || (size_t)rd.start_idx + rd.aligned_string.size() > genome_size)
            throw mat_error("line " + std::to_string(lineno) + ": the aligned read covers " + std::to_string((long long)rd.start_idx + 1) + " .. " +
                            std::to_string((long long)rd.start_idx + (long long)rd.aligned_string.size()) + ", outside the reference 1 .. " +
                            std::to_string(genome_size));
        sink(std::move(rd));
        n++;
    }
    return n;
}
