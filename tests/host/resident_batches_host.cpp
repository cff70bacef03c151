// Stand-alone host program (no device, no HIP call): the argument checks of a batch and the bookkeeping of a batch that
// arrives in blocks (csrc/resident_batches.hpp), driven through the sequences the handles see.  Built with
// -fsanitize=address,undefined by tests/test_cpu_resident_batches.py.
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "resident_batches.hpp"

namespace {

int failures = 0;

template <class F>
void refused(const char* what, const std::string& message, F&& f) {
    try {
        f();
        std::printf("FAIL %s: accepted\n", what);
        ++failures;
    } catch (const bmx::Error& e) {
        if (e.code != BMX_ERR_ARG || message != e.what()) {
            std::printf("FAIL %s: %d '%s'\n", what, e.code, e.what());
            ++failures;
        }
    }
}

// the store's bookkeeping without its device half: what ResidentBatches::begin / add do to the list of batches
struct Ledgers {
    std::vector<std::unique_ptr<bmx::BlockLedger>> batches;
    const bmx::BlockLedger* last() const { return batches.empty() ? nullptr : batches.back().get(); }
    void begin(int64_t n, const int32_t* restrict_idx, int64_t nr) {
        bmx::check_cell_count(n);
        bmx::check_restriction(n, restrict_idx, nr);
        bmx::check_begin(last());
        batches.emplace_back(new bmx::BlockLedger());
        batches.back()->n = n;
    }
    void add(const double* x, int64_t m) {
        bmx::check_block(last(), x, m, "bmx_test_begin_batch");
        batches.back()->filled += m;
    }
};

}  // namespace

int main() {
    std::vector<double> block(16, 0.0);
    const std::vector<int32_t> some = {3, 1, 10, 3}, beyond = {1, 11}, zero = {0};
    Ledgers h;
    refused("block before any batch", "bmx_test_begin_batch has not been called", [&] { h.add(block.data(), 1); });
    // the normal sequence: two batches, the first in three blocks
    h.begin(10, some.data(), (int64_t)some.size());
    h.add(block.data(), 4);
    h.add(block.data(), 4);
    refused("begin before the batch is full", "the previous batch has not received all its cells",
            [&] { h.begin(5, nullptr, -1); });
    refused("a block that does not fit", "the block does not fit into the batch announced", [&] { h.add(block.data(), 3); });
    refused("an empty block", "the block does not fit into the batch announced", [&] { h.add(block.data(), 0); });
    refused("a missing block", "the block is missing", [&] { h.add(nullptr, 2); });
    h.add(block.data(), 2);
    if (!h.last()->complete() || h.batches.size() != 1) ++failures;
    refused("a block after the last", "the block does not fit into the batch announced", [&] { h.add(block.data(), 1); });
    h.begin(1, nullptr, -1);
    h.add(block.data(), 1);
    h.begin(7, some.data(), -1);  // n_restrict < 0: no restriction, the list is not read
    if (h.batches.size() != 3 || h.last()->complete()) ++failures;
    // refused batches leave the list as it was
    refused("no cells", "every batch needs at least one cell", [&] { h.begin(0, nullptr, -1); });
    refused("too many cells", "a batch holds at most 2^31 - 1 cells", [&] { bmx::check_cell_count((int64_t)1 << 31); });
    bmx::check_cell_count((int64_t)1 << 31, false);
    refused("an empty restriction", "no cells remaining in a batch after restriction",
            [&] { bmx::check_restriction(10, some.data(), 0); });
    refused("a restriction beyond the batch", "'restrict' indices out of range",
            [&] { bmx::check_restriction(10, beyond.data(), (int64_t)beyond.size()); });
    refused("a zero-based restriction", "'restrict' indices out of range", [&] { bmx::check_restriction(10, zero.data(), 1); });
    if (h.batches.size() != 3) ++failures;
    std::printf(failures ? "%d failures\n" : "resident batches: host checks ok\n", failures);
    return failures ? 1 : 0;
}
