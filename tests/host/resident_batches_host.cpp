// Stand-alone host program (no device, no HIP call): the argument checks of a batch and the bookkeeping of a batch that
// arrives in blocks, dense or CSC (csrc/resident_batches.hpp), driven through the sequences the handles see, and the
// cutting of a CSC batch into output blocks against the block lists the loop it replaced gave (argv[1]:
// tests/golden/csc_output_blocks_parent.json).  Built with -fsanitize=address,undefined by
// tests/test_cpu_resident_batches.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
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

// what ResidentBatches::begin_csc / add_csc do to the list of batches, in their order
struct CscLedgers {
    std::vector<std::unique_ptr<bmx::CscLedger>> batches;
    const bmx::CscLedger* last() const { return batches.empty() ? nullptr : batches.back().get(); }
    void begin(int64_t n, int64_t nnz) {
        bmx::check_cell_count(n);
        bmx::check_csc_begin(nnz);
        bmx::check_begin(last());
        batches.emplace_back(new bmx::CscLedger());
        batches.back()->n = n;
        batches.back()->nnz = nnz;
    }
    void add(int64_t m, const std::vector<int64_t>& indptr, const int32_t* indices, const double* data) {
        const int64_t nnz = indptr.empty() ? 0 : indptr.back();
        bmx::check_block(last(), indptr.empty() ? nullptr : indptr.data(), m, "bmx_test_begin_batch");
        bmx::CscLedger& b = *batches.back();
        bmx::check_csc_block(b.n, b.filled, m, indptr.data(), indices, data, nnz);
        bmx::check_csc_entries(b, m, nnz);
        b.filled += m;
        b.nnz_filled += nnz;
    }
};

void csc_sequences() {
    const std::vector<int32_t> rows(16, 0);
    const std::vector<double> vals(16, 1.0);
    const int32_t* ri = rows.data();
    const double* va = vals.data();
    CscLedgers h;
    refused("a negative announced nnz", "the batch's number of stored entries is negative", [&] { h.begin(4, -1); });
    refused("csc block before any batch", "bmx_test_begin_batch has not been called", [&] { h.add(1, {0, 1}, ri, va); });
    // six cells with five entries in three blocks, the middle one without a stored entry
    h.begin(6, 5);
    h.add(2, {0, 1, 3}, ri, va);
    h.add(2, {0, 0, 0}, nullptr, nullptr);  // nnz == 0: indices and data may be missing
    refused("begin before the csc batch is full", "the previous batch has not received all its cells", [&] { h.begin(1, 0); });
    refused("the last block one entry short", "the batch has received fewer entries than it announced",
            [&] { h.add(2, {0, 1, 1}, ri, va); });
    refused("the last block one entry over", "the block holds more entries than the batch announced",
            [&] { h.add(2, {0, 1, 3}, ri, va); });
    refused("an early block over", "the block holds more entries than the batch announced", [&] { h.add(1, {0, 3}, ri, va); });
    if (h.last()->filled != 4 || h.last()->nnz_filled != 3) ++failures;  // (a refused block leaves the ledger as it was)
    // check_csc_block's refusals, in its order
    refused("a missing indptr", "the block is missing", [&] { h.add(2, {}, ri, va); });
    refused("a missing indptr (device-free check)", "the block's 'indptr' is missing",
            [&] { bmx::check_csc_block(6, 4, 2, nullptr, ri, va, 0); });
    const int64_t two[3] = {0, 1, 2}, late[3] = {1, 1, 2}, down[3] = {0, 2, 1};
    refused("a negative nnz", "the block's number of stored entries is negative",
            [&] { bmx::check_csc_block(6, 4, 2, two, ri, va, -1); });
    refused("missing indices", "the block's 'indices' or 'data' is missing", [&] { h.add(2, {0, 1, 2}, nullptr, va); });
    refused("missing data", "the block's 'indices' or 'data' is missing", [&] { h.add(2, {0, 1, 2}, ri, nullptr); });
    refused("a csc block that does not fit", "the block does not fit into the batch announced",
            [&] { h.add(3, {0, 1, 2, 2}, ri, va); });
    refused("a block beyond the batch (device-free check)", "the block does not fit into the batch announced",
            [&] { bmx::check_csc_block(6, 5, 2, two, ri, va, 2); });
    refused("indptr that starts late", "the block's 'indptr' does not start at 0",
            [&] { bmx::check_csc_block(6, 4, 2, late, ri, va, 2); });
    refused("indptr that decreases", "the block's 'indptr' decreases", [&] { bmx::check_csc_block(6, 4, 2, down, ri, va, 1); });
    refused("indptr that ends elsewhere", "the block's 'indptr' does not end at its number of stored entries",
            [&] { bmx::check_csc_block(6, 4, 2, two, ri, va, 3); });
    h.add(2, {0, 1, 2}, ri, va);
    if (!h.last()->complete() || h.last()->nnz_filled != 5) ++failures;
    refused("a csc block after the last", "the block does not fit into the batch announced", [&] { h.add(1, {0, 0}, ri, va); });
    h.begin(3, 0);  // a batch without a stored entry
    h.add(3, {0, 0, 0, 0}, nullptr, nullptr);
    if (!h.last()->complete() || h.batches.size() != 2) ++failures;
    // the pattern flags
    const int32_t clean[2] = {0, 0}, row[2] = {1, 1}, order[2] = {0, 1};
    bmx::throw_if_bad_pattern(clean);
    refused("a row outside", "sparse counts: a row index is outside [0, number of genes)", [&] { bmx::throw_if_bad_pattern(row); });
    refused("rows that do not ascend", "sparse counts: the row indices of a column should be strictly ascending",
            [&] { bmx::throw_if_bad_pattern(order); });
}

// Every integer of the file outside its strings, in order: per case n, cap, max_cells, indptr [n + 1], the number of
// blocks, then per block first cell, cells, offset, elements.
void output_blocks_against_parent(const char* path) {
    std::ifstream in(path);
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<int64_t> v;
    bool quoted = false;
    for (size_t i = 0; i < text.size(); ++i) {
        if (text[i] == '"') quoted = !quoted;
        if (quoted || !(text[i] == '-' || (text[i] >= '0' && text[i] <= '9'))) continue;
        char* end = nullptr;
        v.push_back(std::strtoll(text.c_str() + i, &end, 10));
        i = (size_t)(end - text.c_str()) - 1;
    }
    size_t at = 0, cases = 0;
    while (at + 3 <= v.size()) {
        const int64_t n = v[at], cap = v[at + 1], max_cells = v[at + 2];
        const std::vector<int64_t> hp(v.begin() + at + 3, v.begin() + at + 3 + n + 1);
        at += 3 + (size_t)n + 1;
        const size_t nb = (size_t)v[at++];
        const std::vector<bmx::OutBlock> got = bmx::plan_csc_output_blocks(hp.data(), n, cap, max_cells);
        bool same = got.size() == nb;
        for (size_t i = 0; same && i < nb; ++i) {
            const int64_t* w = &v[at + 4 * i];
            same = got[i].bi == 0 && got[i].c0 == w[0] && got[i].mb == w[1] && got[i].at == w[2] && got[i].count == w[3];
        }
        at += 4 * nb;
        if (!same) {
            std::printf("FAIL output blocks, case %zu\n", cases);
            ++failures;
        }
        ++cases;
    }
    if (cases != 6 || at != v.size()) {
        std::printf("FAIL output blocks: %zu cases read\n", cases);
        ++failures;
    }
    // the default limit of cells is that of the loop it replaced
    const int64_t hp[3] = {0, 1, 2};
    if (bmx::plan_csc_output_blocks(hp, 2, 8).size() != 1) ++failures;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: resident_batches_host csc_output_blocks_parent.json\n");
        return 2;
    }
    csc_sequences();
    output_blocks_against_parent(argv[1]);
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
