// Stand-alone driver of the ordered sum (csrc/pt_ordered_sum.hpp, the host template under the tree cost and the convergence monitor) for
// the sanitizer runs of tools/sanitize/run.sh, without a feature around it.  The partial records the bracketing of the sum: its combine is
// a 64-bit hash of both operands, neither commutative nor associative, so any other order, a swapped pair or an entry taken twice changes
// the result.  The expected value is the rule of include/gmupt.h ("Order of a sum") restated here as a loop over levels, strides and
// indices.  Sizes: one run, the padding, a second level, a third level with a padded top run.  CPU only; nothing here touches a device.
#include "../../gmu-path-tracer_amd/csrc/pt_ordered_sum.hpp"

#include <cstdio>
#include <vector>

using namespace gmupt;

struct Bracket { uint64_t h; };

static uint64_t mix(uint64_t z) { z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

static Bracket br_zero() { return Bracket{ 0x243F6A8885A308D3ull }; }
static Bracket br_entry(size_t k) { return Bracket{ mix((uint64_t)k) }; }
static void br_combine(Bracket& x, const Bracket& y) { x.h = mix(x.h * 3u + mix(y.h)); }     // h(x, y) != h(y, x), h(h(x, y), z) != h(x, h(y, z))

// the rule, from the text of the public header
static Bracket restated(size_t n)
{
    std::vector<Bracket> level(n);
    for (size_t k = 0; k < n; k++) level[k] = br_entry(k);
    for (;;) {
        level.resize((level.size() + 255) / 256 * 256, br_zero());                           // padded to a multiple of 256
        for (size_t s = 128; s >= 1; s /= 2)
            for (size_t run = 0; run < level.size(); run += 256)
                for (size_t i = 0; i < s; i++) br_combine(level[run + i], level[run + i + s]);
        std::vector<Bracket> next(level.size() / 256);
        for (size_t r = 0; r < next.size(); r++) next[r] = level[256 * r];
        if (next.size() == 1) return next[0];
        level.swap(next);
    }
}

int main()
{
    Bracket x12 = br_entry(1), x21 = br_entry(2), x23 = br_entry(2), right = br_entry(1);
    br_combine(x12, br_entry(2)); br_combine(x21, br_entry(1));                              // h(1, 2), h(2, 1)
    Bracket left = x12;
    br_combine(left, br_entry(3));                                                           // h(h(1, 2), 3)
    br_combine(x23, br_entry(3)); br_combine(right, x23);                                    // h(1, h(2, 3))
    if (x12.h == x21.h || left.h == right.h) { std::fprintf(stderr, "ordered sum: the test's combine does not tell the orders apart\n"); return 1; }
    const size_t sizes[] = { 1, 2, 255, 256, 257, 65536, 65537 };
    for (size_t n : sizes) {
        const Bracket want = restated(n);
        for (int threads : { 1, 8 }) {
            const Bracket got = ordered_sum_host<br_zero, br_combine>(n, threads, br_entry);
            if (got.h != want.h) {
                std::fprintf(stderr, "ordered sum: %zu entries, %d threads: %016llx, the restated rule gives %016llx\n", n, threads,
                             (unsigned long long)got.h, (unsigned long long)want.h);
                return 1;
            }
        }
        std::printf("ordered sum %zu entries: %016llx at 1 and 8 threads\n", n, (unsigned long long)want.h);
    }
    return 0;
}
