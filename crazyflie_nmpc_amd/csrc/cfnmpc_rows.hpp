// cfnmpc_rows.hpp -- per-vehicle arrays of the fleet and multi-GPU layers: the description of one array of a call (Col), the
// layout of a call's columns in a staging area, and the plain host code that moves their rows between the fleet's vehicle
// order and the order of a bucket or shard.  Plain C++, no HIP (tools/host_rows_check.cpp runs it under the host sanitizers).
// Internal to the library; DESIGN.md section 5.19.
#pragma once
#include <cassert>
#include <cstddef>
#include <cstring>
#include <initializer_list>

namespace cfn {

// One array of a fleet-level call: `len` elements per vehicle (per STAGE and vehicle for yref and the stage boxes: a bucket of
// horizon N then holds len * N per row, and the fleet's rows are len * Nmax apart).  p = nullptr: not requested.
struct Col {
    void* p;
    size_t esz;       // sizeof(double) or sizeof(int)
    size_t len;
    bool per_stage;
};
inline Col col(const double* p, size_t len) { return {const_cast<double*>(p), sizeof(double), len, false}; }
inline Col col(const int* p, size_t len) { return {const_cast<int*>(p), sizeof(int), len, false}; }
inline Col col_stages(const double* p, size_t len) { return {const_cast<double*>(p), sizeof(double), len, true}; }

constexpr int MAX_COLS = 4;
using Cols = std::initializer_list<Col>;

// The columns of one call for `count` vehicles of horizon N out of a fleet whose longest horizon is Nmax: row length and fleet
// stride of every column, and its place in a staging area -- the requested columns one after another, each starting on a
// multiple of 8 bytes (so that ints and doubles are aligned whatever precedes them).
struct Layout {
    int n = 0;
    Col c[MAX_COLS];
    size_t len[MAX_COLS], stride[MAX_COLS], off[MAX_COLS];
    size_t bytes = 0;

    Layout(Cols cols, size_t count, int N, int Nmax) {
        assert(cols.size() <= (size_t)MAX_COLS);
        for (const Col& k : cols) {
            c[n] = k;
            len[n] = k.per_stage ? k.len * N : k.len;
            stride[n] = k.per_stage ? k.len * Nmax : k.len;
            off[n] = bytes;
            if (k.p) bytes += (count * len[n] * k.esz + 7) / 8 * 8;
            n++;
        }
    }
    // the column's place in the staging area at `base` (nullptr for a column not requested)
    void* at(void* base, int i) const { return c[i].p ? static_cast<char*>(base) + off[i] : nullptr; }
    // the column's rows from vehicle `lo` on in the caller's array: what a CONTIGUOUS shard reads or writes in place
    void* from(int i, size_t lo) const { return c[i].p ? static_cast<char*>(c[i].p) + lo * stride[i] * c[i].esz : nullptr; }
};

// the staged columns of one call, as the callee takes them
struct Staged {
    void* p[MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};
    double* d(int i) const { return static_cast<double*>(p[i]); }
    int* i(int k) const { return static_cast<int*>(p[k]); }
};
inline Staged staged(const Layout& L, void* base) {
    Staged s;
    for (int i = 0; i < L.n; i++) s.p[i] = L.at(base, i);
    return s;
}
inline Staged in_place(const Layout& L, size_t lo) {
    Staged s;
    for (int i = 0; i < L.n; i++) s.p[i] = L.from(i, lo);
    return s;
}

// host arrays, every requested column: staging row r <- the caller's row idx[r] (GATHER), or the caller's row idx[r] <- staging
// row r (!GATHER)
template <bool GATHER>
void move_rows(const Layout& L, void* base, const int* idx, size_t count) {
    for (int i = 0; i < L.n; i++) {
        if (!L.c[i].p) continue;
        const size_t row = L.len[i] * L.c[i].esz, frow = L.stride[i] * L.c[i].esz;
        char* sg = static_cast<char*>(L.at(base, i)), *fl = static_cast<char*>(L.c[i].p);
        for (size_t r = 0; r < count; r++) {
            if (GATHER) std::memcpy(sg + r * row, fl + (size_t)idx[r] * frow, row);
            else std::memcpy(fl + (size_t)idx[r] * frow, sg + r * row, row);
        }
    }
}

}  // namespace cfn
