// Host-side driver of csrc/merge_plan.hpp for tests/test_cpu_merge_plan.py: no HIP header, no device.  Built with a plain C++
// compiler under AddressSanitizer and UndefinedBehaviorSanitizer.  One case per line of standard input, one JSON line out:
//   tree B c...        the post-order code c of B batches, batch b (1-based) of b cells
//   restrict n i...    the 1-based restrict vector i of a batch of n cells
//   counts R v...      the R x R count matrix v (row-major): .pick_best_merge and the matrix of .update_remainders
// An error of the header comes out as {"error": code, "text": message}.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "merge_plan.hpp"

using namespace bmx;

namespace {

template <class T>
std::string list(const std::vector<T>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s + "]";
}

void leaves_of(const MergePlan& P, int at, std::vector<int>& out) {
    if (P.nodes[at].batch >= 0) {
        out.push_back(P.nodes[at].batch + 1);
        return;
    }
    leaves_of(P, P.nodes[at].left, out);
    leaves_of(P, P.nodes[at].right, out);
}

std::string side(const MergePlan& P, int at) {
    std::vector<int> lv;
    leaves_of(P, at, lv);
    return "{\"leaf\":" + std::string(P.nodes[at].batch >= 0 ? "true" : "false") + ",\"batches\":" + list(lv) +
           ",\"row0\":" + std::to_string(P.nodes[at].row0) + ",\"n\":" + std::to_string(P.nodes[at].n) + "}";
}

std::string run_case(const std::string& kind, const std::vector<int32_t>& v) {
    if (kind == "tree") {
        const int B = v.at(0);
        std::vector<int32_t> nrows;
        for (int b = 1; b <= B; ++b) nrows.push_back(b);
        const MergePlan P = plan_merges(v.data() + 1, (int)v.size() - 1, B, nrows.data());
        std::string s = "{\"merges\":[";
        for (size_t m = 0; m < P.merges.size(); ++m) {
            const PlanNode& x = P.nodes[P.merges[m]];
            s += (m ? "," : "") + std::string("{\"left\":") + side(P, x.left) + ",\"right\":" + side(P, x.right) +
                 ",\"row0\":" + std::to_string(x.row0) + ",\"n\":" + std::to_string(x.n) + "}";
        }
        std::vector<int> need;
        for (int b : P.need_order) need.push_back(b + 1);
        return s + "],\"need\":" + list(need) + ",\"root\":" + std::to_string(P.merges.empty() ? -1 : P.merges.back()) +
               ",\"nodes\":" + std::to_string(P.nodes.size()) + "}";
    }
    if (kind == "restrict") {
        const int n = v.at(0), m = (int)v.size() - 1;
        const RestrictChains c = restrict_chains(v.data() + 1, m, n, 1);
        return "{\"rows\":" + list(c.rows) + ",\"next\":" + list(std::vector<int32_t>(c.next(), c.next() + m)) +
               ",\"head\":" + list(std::vector<int32_t>(c.head(), c.head() + m)) + ",\"dups\":" + (c.dups ? "true" : "false") +
               "}";
    }
    if (kind == "counts") {
        const int R = v.at(0);
        CountMatrix st((size_t)R, std::vector<int64_t>((size_t)R, 0));
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < R; ++j) st[i][j] = v.at((size_t)1 + i * R + j);
        const BestMerge b = pick_best_merge(st);
        std::vector<int> keep;
        const CountMatrix ns = drop_merged(st, b.left, b.right, keep);
        std::string s = "{\"left\":" + std::to_string(b.left) + ",\"right\":" + std::to_string(b.right) +
                        ",\"count\":" + std::to_string(b.count) + ",\"keep\":" + list(keep) + ",\"next\":[";
        for (size_t i = 0; i < ns.size(); ++i) s += (i ? "," : "") + list(ns[i]);
        return s + "]}";
    }
    throw std::runtime_error("unknown case " + kind);
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        std::vector<int32_t> v;
        for (int32_t x; in >> x;) v.push_back(x);
        try {
            std::printf("%s\n", run_case(kind, v).c_str());
        } catch (const Error& e) {
            std::printf("{\"error\":%d,\"text\":\"%s\"}\n", e.code, e.what());
        }
    }
    std::printf("merge plan cases done\n");
    return 0;
}
