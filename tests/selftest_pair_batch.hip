// Host self-test of the pair entries' launch plumbing (gt4py_amd/csrc/field_args.hip.h): next_pair_batch, shared_field,
// with_pair_entries and with_item_type write into and choose between fixed-size things, so they run here on heap arrays that are
// exactly as large as a call says, under -fsanitize=address,undefined (tests/test_c_abi.py builds and runs this; no GPU, no HIP
// call).  Every address is made up and never read through.
#include <cstdio>
#include <cstring>
#include <memory>
#include <type_traits>

#include "field_args.hip.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

// the shape of the entries' args structs, with guards around what a batch may write
struct Args {
    unsigned char before[32];
    gt4mi::PairEntry e[gt4mi::PAIR_MAX_FIELDS];
    unsigned char after[32];
    int nf;
};

constexpr int SIZE = 8;

// field n of side `side` (0 written, 1 read): everything differs between fields, sides and axes
gt4mi_field field(int side, int n) {
    gt4mi_field f{};
    f.data = reinterpret_cast<void*>((uintptr_t)(0x100000 * (side + 1) + 0x1000 * n));
    for (int ax = 0; ax < 3; ++ax) {
        f.shape[ax] = 16;
        f.stride[ax] = SIZE * (1 + ax + 3 * n + 100 * side) * (ax == 1 ? -1 : 1);
        f.origin[ax] = 1 + ax + side;
    }
    return f;
}

void expect_entry(const gt4mi::PairEntry& e, const gt4mi_field& d, const gt4mi_field& s, const int* order) {
    EXPECT(e.dst == gt4mi::origin_ptr(d) && e.src == gt4mi::origin_ptr(s));
    for (int x = 0; x < 3; ++x) {
        const int ax = order != nullptr ? order[x] : x;
        EXPECT(e.d[x] == d.stride[ax] / SIZE && e.s[x] == s.stride[ax] / SIZE);
    }
}

void check_call(int nfields, const int* order) {
    // heap arrays of exactly nfields descriptors: a read past the call's pairs is a heap-buffer-overflow
    std::unique_ptr<gt4mi_field[]> dst(new gt4mi_field[nfields]), src(new gt4mi_field[nfields]);
    for (int n = 0; n < nfields; ++n) dst[n] = field(0, n), src[n] = field(1, n);
    const gt4mi::PairEntry zero{};
    for (int first = 0; first <= nfields; ++first) {  // every start, not only the multiples of PAIR_MAX_FIELDS the loop reaches
        Args a;
        std::memset(&a, 0xAB, sizeof a);
        int next = first;
        const bool more = gt4mi::next_pair_batch(a, dst.get(), src.get(), &next, nfields, SIZE, order);
        EXPECT(more == (first < nfields));
        if (!more) {
            EXPECT(next == first);
            continue;
        }
        const int left = nfields - first, nf = left < gt4mi::PAIR_MAX_FIELDS ? left : gt4mi::PAIR_MAX_FIELDS;
        EXPECT(a.nf == nf && next == first + nf);
        for (int n = 0; n < nf; ++n) expect_entry(a.e[n], dst[first + n], src[first + n], order);
        for (int n = nf; n < gt4mi::PAIR_MAX_FIELDS; ++n) EXPECT(std::memcmp(&a.e[n], &zero, sizeof zero) == 0);
        for (unsigned char c : a.before) EXPECT(c == 0xAB);
        for (unsigned char c : a.after) EXPECT(c == 0xAB);
    }
    // the loop as the entries write it: every pair once, in order, ceil(nfields / 8) launches
    Args a{};
    int next = 0, launches = 0, seen = 0;
    while (gt4mi::next_pair_batch(a, dst.get(), src.get(), &next, nfields, SIZE, order)) {
        for (int n = 0; n < a.nf; ++n) EXPECT(a.e[n].dst == gt4mi::origin_ptr(dst[seen + n]));
        seen += a.nf, ++launches;
    }
    EXPECT(seen == nfields && launches == (nfields + gt4mi::PAIR_MAX_FIELDS - 1) / gt4mi::PAIR_MAX_FIELDS);
}

}  // namespace

int main() {
    static_assert(sizeof(gt4mi::PairEntry) == 64 && sizeof(gt4mi::SharedField) == 32, "the kernels' argument layout");
    static_assert(std::is_trivially_copyable<gt4mi::PairEntry>::value && std::is_trivially_copyable<gt4mi::SharedField>::value, "");
    const int orders[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int nfields : {1, 4, 5, 8, 9, 16, 17}) {
        check_call(nfields, nullptr);
        for (const auto& order : orders) check_call(nfields, order);
    }
    // shared_field: the origin item and the strides, in the order asked for
    const gt4mi_field f = field(1, 3);
    for (const auto& order : orders) {
        const gt4mi::SharedField q = gt4mi::shared_field(f, SIZE, order);
        EXPECT(q.p == gt4mi::origin_ptr(f));
        for (int x = 0; x < 3; ++x) EXPECT(q.s[x] == f.stride[order[x]] / SIZE);
    }
    const gt4mi::SharedField plain = gt4mi::shared_field(f, SIZE);
    for (int x = 0; x < 3; ++x) EXPECT(plain.s[x] == f.stride[x] / SIZE);
    // the instantiation of a batch: 1 -> 1, 2 .. 4 -> 4, 5 .. 8 -> 8
    for (int nf = 1; nf <= gt4mi::PAIR_MAX_FIELDS; ++nf) {
        int got = 0, calls = 0;
        gt4mi::with_pair_entries(nf, [&](auto n) { got = decltype(n)::value, ++calls; });
        EXPECT(calls == 1 && got == (nf == 1 ? 1 : nf <= 4 ? 4 : 8) && got >= nf);
    }
    for (int size : {4, 8}) {
        int got = 0;
        gt4mi::with_item_type(size, [&](auto t) { got = (int)sizeof(t) + (std::is_floating_point<decltype(t)>::value ? 0 : 100); });
        EXPECT(got == size);
    }
    if (failures != 0) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("pair batch plumbing: clean under the sanitizers\n");
    return 0;
}
