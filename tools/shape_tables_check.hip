// shape_tables_check.hip - the table walkers of csrc/handle.h over every row of every table of csrc/shapes.h, as a stand-alone host
// program for a sanitizer build (no GPU is touched, nothing is loaded into Python):
//     hipcc --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/shape_tables_check.hip -o shape_tables_check
// For a handle of each row's shape every walker must call fn exactly once, with that row's constants; for a stack the one-layer
// walkers, and for a shape outside a table every walker, must return false without calling fn.
#include <cstdio>
#include <cstdlib>

#include "../rnnwavefunctions_amd/csrc/shapes.h"

using namespace rnnwf;

namespace {

int checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++checks;                                                                \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

struct Seen {
    int calls = 0;
    bool f64 = false;
    int nl = 0, nfull = 0, waves = 0, nf32 = -1, rj = -1, mode = -1;
    bool is(bool f64_, int nl_, int nfull_, int waves_) const { return calls == 1 && f64 == f64_ && nl == nl_ && nfull == nfull_ && waves == waves_; }
};
template <typename T, int NFULL, int NL, int WAVES> struct K4 {
    static void see(Seen& s) { ++s.calls; s.f64 = std::is_same<T, double>::value; s.nl = NL; s.nfull = NFULL; s.waves = WAVES; }
};
template <typename T, int NFULL, int WAVES> struct K3 : K4<T, NFULL, 1, WAVES> {};
template <int NFULL, int WAVES> struct K2 {
    static void see(Seen& s) { ++s.calls; s.nl = 1; s.nfull = NFULL; s.waves = WAVES; }
};

rnnwf_handle* shape(bool f64, int nl, int nfull, int H) {
    rnnwf_handle* h = new rnnwf_handle();                   // (freed by the caller: the leak checker runs too)
    h->f64 = f64;
    h->NL = nl;
    h->NFULL = nfull;
    h->H = H;
    return h;
}

template <class F, class... Rows>
void each_row(KernelTable<Rows...>, F&& f) { (f(Rows()), ...); }

// every walker on a handle that has no row in Table
template <class Table>
void refused(Table t, bool f64, int nl, int nfull, int H) {
    rnnwf_handle* h = shape(f64, nl, nfull, H);
    Seen s;
    CHECK(!with_row(t, h, [&](auto) { ++s.calls; }));
    CHECK(!with_layer_kernels<K3>(t, h, [&](auto k) { decltype(k)::see(s); }));
    CHECK(!with_width_kernels<K2>(t, h, [&](auto k) { decltype(k)::see(s); }));
    CHECK(s.calls == 0);
    delete h;
}

// a table of KernelRow: with_row, with_kernels, with_layer_kernels, with_width_kernels on every row's shape
template <class Table>
int kernel_table(Table t) {
    int rows = 0;
    each_row(t, [&](auto row) {
        using R = decltype(row);
        constexpr bool f64 = std::is_same<typename R::T, double>::value;
        rnnwf_handle* h = shape(f64, R::NL, R::NFULL, 16 * R::NFULL + 4);
        ++rows;
        Seen a, b, c, d;
        CHECK(with_row(t, h, [&](auto r) { K4<typename decltype(r)::T, decltype(r)::NFULL, decltype(r)::NL, decltype(r)::WAVES>::see(a); }));
        CHECK(a.is(f64, R::NL, R::NFULL, R::WAVES));
        CHECK(with_kernels<K4>(t, h, [&](auto k) { decltype(k)::see(b); }));
        CHECK(b.is(f64, R::NL, R::NFULL, R::WAVES));
        const bool one = R::NL == 1;
        CHECK(with_layer_kernels<K3>(t, h, [&](auto k) { decltype(k)::see(c); }) == one);
        CHECK(one ? c.is(f64, 1, R::NFULL, R::WAVES) : c.calls == 0);
        CHECK(with_width_kernels<K2>(t, h, [&](auto k) { decltype(k)::see(d); }) == one);
        CHECK(one ? d.is(false, 1, R::NFULL, R::WAVES) : d.calls == 0);
        delete h;
        // the same shape in the other element type, and with a layer more than any table has, belongs to another row or to none
        rnnwf_handle* o = shape(!f64, R::NL, R::NFULL, 16 * R::NFULL + 4);
        Seen e;
        with_kernels<K4>(t, o, [&](auto k) { decltype(k)::see(e); });
        CHECK(e.calls == 0 || e.is(!f64, R::NL, R::NFULL, e.waves));
        delete o;
        refused(t, f64, RNNWF_MAX_LAYERS + 1, R::NFULL, 16 * R::NFULL + 4);
    });
    return rows;
}

// the bf16x3 table: both ends of every row's range of unit counts
int split_table() {
    int rows = 0;
    each_row(SplitKernels(), [&](auto row) {
        using R = decltype(row);
        ++rows;
        const int lo = std::max(R::HMIN, 16 * (R::NFULL - 1) + 5), hi = std::min(R::HMAX, 16 * R::NFULL + 4);
        CHECK(lo <= hi);
        for (int H : {lo, hi}) {
            rnnwf_handle* h = shape(false, 1, R::NFULL, H);
            Seen s;
            CHECK(with_row(SplitKernels(), h, [&](auto r) {
                using Q = decltype(r);
                ++s.calls; s.nfull = Q::NFULL; s.waves = Q::WAVES; s.nf32 = Q::NF32; s.rj = Q::RJ; s.mode = Q::MODE;
            }));
            CHECK(s.calls == 1 && s.nfull == R::NFULL && s.waves == R::WAVES && s.nf32 == R::NF32 && s.rj == R::RJ && s.mode == R::MODE);
            delete h;
        }
    });
    return rows;
}

}  // namespace

int main() {
    static_assert(kGru1Waves<double, 4, 8> == 4 && kGru1Waves<double, 6, 4> == 4 && kGru1Waves<float, 6, 8> == 8 && kGru1Waves<float, 4, 4> == 4,
                  "the observable passes' one exception");
    CHECK(kernel_table(GruKernels()) == 40);
    CHECK(kernel_table(CrnnKernels()) == 23);
    CHECK(kernel_table(MdKernels()) == 5);
    CHECK(kernel_table(LstmKernels()) == 4);
    CHECK(kernel_table(BaseBfKernels()) == 3);
    CHECK(split_table() == 6);
    // one step past each table's last row, and the gaps inside
    refused(GruKernels(), true, 1, 8, 132);                 // f64 GRU: one layer stops at NFULL 6 ...
    refused(GruKernels(), true, 2, 6, 69);                  // ... its stacks at 4
    refused(GruKernels(), false, 2, 8, 101);                // f32 stacks stop at 6
    refused(GruKernels(), false, 1, 5, 84);                 // no width class 5, 7, 20
    refused(GruKernels(), false, 1, 7, 116);
    refused(GruKernels(), false, 1, 20, 324);
    refused(GruKernels(), false, 0, 1, 20);
    refused(CrnnKernels(), true, 1, 1, 20);                 // f32 only
    refused(CrnnKernels(), false, 2, 8, 101);
    refused(CrnnKernels(), false, 1, 20, 324);
    refused(MdKernels(), true, 1, 6, 85);
    refused(MdKernels(), true, 2, 1, 20);
    refused(MdKernels(), false, 1, 1, 20);
    refused(LstmKernels(), true, 1, 5, 69);
    refused(LstmKernels(), true, 1, 6, 69);
    refused(BaseBfKernels(), false, 1, 4, 53);
    refused(BaseBfKernels(), false, 2, 3, 50);
    refused(BaseBfKernels(), true, 1, 3, 50);
    for (int nfull : {0, 5, 8, 12, 16}) {
        rnnwf_handle* h = shape(false, 1, nfull, 16 * nfull + 4);
        CHECK(!with_row(SplitKernels(), h, [&](auto) { CHECK(false); }));
        delete h;
    }
    printf("shape tables: %d checks passed\n", checks);
    return 0;
}
