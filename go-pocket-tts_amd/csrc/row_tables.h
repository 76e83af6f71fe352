// row_tables.h -- how a list of rows is cut into the tables of the post-processing kernels (dsp_device.cpp): the one
// statement of the rule, for the DSP table's equalisers, the compressor's designs and the limiter's.  No HIP header: a plain compiler builds it
// (tests/test_row_tables_cpu.py does, with sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ptts {

// Rows [0, key.size()) in order into tables of at most max_rows rows and at most max_designs distinct designs each.  key[i] is row i's design
// (null: the row names none and fits any table); same(a, b) says whether two designs are one; both limits are at least 1.  Greedy: a row goes into the running table
// unless the table is full or the row would bring its design number max_designs + 1, and then it starts the next one.
// table(first, count, index, designs) is called for each table in order: rows [first, first + count), index[k] the place of row first + k's
// design among `designs` (0 for a row without one), designs the table's distinct ones in first-use order.
template <class Design, class Same, class Table>
inline void cut_tables(const std::vector<const Design*>& key, int max_rows, int max_designs, Same&& same, Table&& table) {
    std::vector<const Design*> designs;
    std::vector<int32_t> index;
    for (size_t first = 0; first < key.size();) {
        designs.clear();
        index.clear();
        for (size_t i = first; i < key.size() && index.size() < (size_t)max_rows; i++) {
            size_t k = 0;
            if (key[i]) {
                while (k < designs.size() && !same(*designs[k], *key[i])) k++;
                if (k == designs.size()) {
                    if (designs.size() == (size_t)max_designs) break;   // the next table's
                    designs.push_back(key[i]);
                }
            }
            index.push_back((int32_t)k);
        }
        table(first, (int)index.size(), index.data(), designs);
        first += index.size();
    }
}

}  // namespace ptts
