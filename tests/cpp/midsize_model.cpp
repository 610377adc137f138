// midsize_model.cpp — host restatement of K2V's mid-size phase (csrc/align_refv.hip), checked against the
// real std::nth_element of this toolchain (test infrastructure; tests/test_k2v_midsize.py builds and runs it).
//
// The device runs libstdc++'s introselect as parallel Hoare rounds (tests/cpp/introselect_model.cpp has the round
// form and its proof sketch).  Block rounds work on the register-resident vector while the segment is larger than MID;
// a segment of OW < S <= MID positions is copied once to a buffer of its own (position first + i at index i), its
// rounds run there on relative positions (nth relative too), vec[nth - 1] is recorded at the round that cuts exactly
// at nth (the one value the result may need from outside a later segment), and once S <= OW the kept part moves to
// index 0 of the buffer for the one-wave rounds.  The depth limit counts every round of every phase; when it runs out
// the heap select takes whatever segment is current, inside the phase too.
//
// For every input the program takes median and MAD (src/algorithm.cpp:834-865 of the reference: nth_element at n / 2,
// the mean with vec[n / 2 - 1] for an even length) through this flow and through std::nth_element and requires the
// same vec[nth - 1], vec[nth], median and MAD bit for bit.  Prints "ok <cases> <cases that ran mid-size rounds>
// <cases that took the heap select inside or after the phase>" or the first mismatch.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using V = double;

// ---- heap select, restated (stl_heap.h / stl_algo.h __heap_select), as in introselect_model.cpp
static void push_heap_m(V* a, long hole, long top, V value) {
    long parent = (hole - 1) / 2;
    while (hole > top && a[parent] < value) {
        a[hole] = a[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    a[hole] = value;
}
static void adjust_heap_m(V* a, long hole, long len, V value) {
    const long top = hole;
    long second = hole;
    while (second < (len - 1) / 2) {
        second = 2 * (second + 1);
        if (a[second] < a[second - 1]) second--;
        a[hole] = a[second];
        hole = second;
    }
    if ((len & 1) == 0 && second == (len - 2) / 2) {
        second = 2 * (second + 1);
        a[hole] = a[second - 1];
        hole = second - 1;
    }
    push_heap_m(a, hole, top, value);
}
static void heap_select_m(V* first, long middle, long last) {
    if (middle >= 2) {
        long parent = (middle - 2) / 2;
        while (true) {
            adjust_heap_m(first, parent, middle, first[parent]);
            if (parent == 0) break;
            parent--;
        }
    }
    for (long i = middle; i < last; ++i)
        if (first[i] < first[0]) {
            const V value = first[i];
            first[i] = first[0];
            adjust_heap_m(first, 0, middle, value);
        }
}

// ---- one round in the parallel form on a[first, last); returns cut
static long round_pf(std::vector<V>& a, long first, long last) {
    const long S = last - first;
    const long A = first + 1, B = first + S / 2, C = last - 1;
    long ch;
    if (a[A] < a[B]) ch = a[B] < a[C] ? B : (a[A] < a[C] ? C : A);
    else ch = a[A] < a[C] ? A : (a[B] < a[C] ? C : B);
    std::swap(a[first], a[ch]);
    const V p = a[first];
    std::vector<long> ge, le;
    for (long i = first + 1; i < last; ++i)
        if (!(a[i] < p)) ge.push_back(i);
    for (long i = last - 1; i >= first; --i)
        if (!(p < a[i])) le.push_back(i);
    long ks = 0, g = 0, lc = (long)le.size() - 1;  // t = first + 1 (position first holds p: an LE)
    for (long t = first + 1; t <= last; ++t) {
        ks = std::max(ks, std::min(g, lc));
        if (t < last) {
            if (!(a[t] < p)) ++g;
            if (!(p < a[t])) --lc;
        }
    }
    long cut = (long)ge.size() > ks ? ge[ks] : LONG_MAX;
    if (ks > 0) cut = std::min(cut, le[ks - 1]);
    for (long k = 0; k < ks; ++k) std::swap(a[ge[k]], a[le[k]]);
    return cut;
}

static int lg(long n) { int r = 0; while (n >>= 1) ++r; return r; }

struct Sel {
    V hi = 0, lo = 0;
    int nmid = 0;
    bool heap = false, entered = false;
};

// std::nth_element(a, a + nth) the device's way; hi = vec[nth], lo = vec[nth - 1] (nth >= 1)
static Sel select_dev(std::vector<V> a, long nth, long OW, long MID) {
    Sel r;
    long first = 0, last = (long)a.size();
    int depth = last > 1 ? 2 * lg(last) : 0;
    bool rec = false;
    // the heap select on seg[f, l) (positions base + f ..), nth at relative position nr
    auto finish_heap = [&](std::vector<V>& seg, long f, long l, long nr) {
        heap_select_m(seg.data() + f, nr + 1 - f, l - f);
        std::swap(seg[f], seg[nr]);
        r.heap = true;
        r.hi = seg[nr];
        if (!rec && nth >= 1) r.lo = seg[nr - 1];  // (nr - 1 >= f: nr == f only after a recorded cut, or at 0)
    };
    while (last - first > MID && depth > 0) {  // block rounds
        --depth;
        const long cut = round_pf(a, first, last);
        if (cut == nth && !rec && nth >= 1) { r.lo = a[nth - 1]; rec = true; }
        if (cut <= nth) first = cut;
        else last = cut;
    }
    if (last - first > OW && depth == 0) {  // depth limit before the phase
        finish_heap(a, first, last, nth);
        return r;
    }
    long base = 0;            // position of seg[0]
    std::vector<V> seg;
    long f, l;
    if (last - first > OW) {  // the mid-size phase: dump, rounds on relative positions
        r.entered = true;
        base = first;
        seg.assign(a.begin() + first, a.begin() + last);
        f = 0;
        l = last - first;
        const long nr = nth - base;
        while (l - f > OW && depth > 0) {
            --depth;
            ++r.nmid;
            const long cut = round_pf(seg, f, l);
            if (cut == nr && !rec && nth >= 1) { r.lo = seg[nr - 1]; rec = true; }
            if (cut <= nr) f = cut;
            else l = cut;
        }
        if (l - f > OW) {  // depth limit inside the phase
            finish_heap(seg, f, l, nr);
            return r;
        }
        // hand-over: the kept part to index 0
        std::vector<V> s2(seg.begin() + f, seg.begin() + l);
        base += f;
        seg.swap(s2);
    } else {
        base = first;
        seg.assign(a.begin() + first, a.begin() + last);
    }
    f = 0;
    l = (long)seg.size();
    const long nr = nth - base;
    while (l - f > 3 && depth > 0) {  // one-wave and one-row rounds
        --depth;
        const long cut = round_pf(seg, f, l);
        if (cut == nr && !rec && nth >= 1) { r.lo = seg[nr - 1]; rec = true; }
        if (cut <= nr) f = cut;
        else l = cut;
    }
    if (l - f > 3) {
        finish_heap(seg, f, l, nr);
        return r;
    }
    std::sort(seg.begin() + f, seg.begin() + l);
    r.hi = seg[nr];
    if (!rec && nth >= 1) r.lo = seg[nr - 1];
    return r;
}

static long g_cases = 0, g_mid = 0, g_heap = 0;

static V median_of(V lo, V hi, long n, long nth) { return (n % 2 == 0 && nth >= 1) ? (lo + hi) / 2.0 : hi; }

// one pass: the device flow against std::nth_element; returns the median through `med`
static bool check_pass(const std::vector<V>& in, long nth, long OW, long MID, const char* what, V* med, bool expect_mid) {
    std::vector<V> ref(in);
    std::nth_element(ref.begin(), ref.begin() + nth, ref.end());
    const Sel s = select_dev(in, nth, OW, MID);
    ++g_cases;
    g_mid += s.nmid > 0;
    g_heap += s.heap && s.entered;
    const long n = (long)in.size();
    if (!(s.hi == ref[nth]) || (nth >= 1 && !(s.lo == ref[nth - 1]))) {
        std::printf("MISMATCH %s n=%ld nth=%ld OW=%ld MID=%ld: hi %.17g vs %.17g, lo %.17g vs %.17g\n", what, n, nth, OW, MID,
                    s.hi, ref[nth], s.lo, nth >= 1 ? ref[nth - 1] : 0.0);
        return false;
    }
    if (expect_mid && !s.entered) {
        std::printf("NO MID PHASE %s n=%ld nth=%ld OW=%ld MID=%ld\n", what, n, nth, OW, MID);
        return false;
    }
    *med = median_of(s.lo, s.hi, n, nth);
    const V mref = median_of(nth >= 1 ? ref[nth - 1] : 0.0, ref[nth], n, nth);
    if (!(*med == mref)) {
        std::printf("MISMATCH %s n=%ld nth=%ld: median %.17g vs %.17g\n", what, n, nth, *med, mref);
        return false;
    }
    return true;
}
// median, then MAD on |v - median| in the original order (DBL_MAX stays DBL_MAX)
static bool check(const std::vector<V>& v, long nvis, long OW, long MID, const char* what, bool expect_mid) {
    const long nth = nvis / 2;
    V med = 0, mad = 0;
    if (!check_pass(v, nth, OW, MID, what, &med, expect_mid)) return false;
    std::vector<V> d(v.size());
    for (size_t i = 0; i < v.size(); ++i) d[i] = v[i] >= DBL_MAX ? DBL_MAX : std::fabs(v[i] - med);
    return check_pass(d, nth, OW, MID, what, &mad, false);
}

static std::vector<V> content(int kind, long n, std::mt19937_64& rng, long* nvis) {
    std::vector<V> v(n);
    std::normal_distribution<double> nd(0.0, 8.0);
    *nvis = n;
    switch (kind) {
        case 0: {  // residual-like, 20 % DBL_MAX in groups of 25
            for (auto& x : v) x = nd(rng);
            long vis = 0;
            for (long f = 0; f * 25 < n; ++f) {
                const bool hide = std::uniform_real_distribution<double>(0, 1)(rng) < 0.2;
                for (long k = f * 25; k < std::min(n, f * 25 + 25); ++k) {
                    if (hide) v[k] = DBL_MAX;
                    else ++vis;
                }
            }
            if (vis == 0) { v[0] = 0.0; vis = 1; }
            *nvis = vis;
            break;
        }
        case 1: for (auto& x : v) x = std::round(nd(rng) * 0.5); break;  // small integers
        case 2: for (auto& x : v) x = 3.0; break;                         // all equal
        case 3: for (long i = 0; i < n; ++i) v[i] = (V)i; break;          // ascending
        case 4: for (long i = 0; i < n; ++i) v[i] = (V)(n - i); break;    // descending
        case 5: {                                                         // organ pipe
            const long h = (n + 1) / 2;
            for (long i = 0; i < n; ++i) v[i] = (V)(i < h ? i : n - 1 - i);
            break;
        }
        case 6: for (auto& x : v) x = (rng() & 1) ? 0.0 : -0.0; break;    // +-0.0 mixed
        default: {                                                        // one visible slot
            for (auto& x : v) x = DBL_MAX;
            v[(size_t)(rng() % (unsigned long)n)] = 1.5;
            *nvis = 1;
            break;
        }
    }
    return v;
}

int main(int argc, char** argv) {
    const long trials = argc > 1 ? std::atol(argv[1]) : 2000;
    std::mt19937_64 rng(2468);
    // the product's and the debug kernel's sizes, and small ones that put short random vectors through every branch
    const long cfg[][2] = {{2048, 7168}, {1024, 7168}, {2048, 4096}};
    for (const auto& c : cfg) {
        const long OW = c[0], MID = c[1];
        for (long n : {OW + 1, OW + 2, MID - 1, MID, MID + 1, 4097L, 5000L, 9000L})
            for (int kind = 0; kind < 8; ++kind) {
                long nvis;
                const std::vector<V> v = content(kind, n, rng, &nvis);
                char what[64];
                std::snprintf(what, sizeof what, "family %d", kind);
                // (the phase is entered whenever a segment of OW < S <= MID still has rounds left: always for n <= MID)
                if (!check(v, nvis, OW, MID, what, n <= MID)) return 1;
                // every nth position class: first, last, middle
                for (long nv : {2L, 2 * n / 3, n}) {
                    if (!check(v, std::min(nv, n), OW, MID, what, false)) return 1;
                }
            }
    }
    for (long t = 0; t < trials; ++t) {  // random short vectors on small phase sizes
        const long OW = 8 << (rng() % 4), MID = OW + 8 * (1 + (long)(rng() % 12));
        const long n = 4 + (long)(rng() % 400);
        std::vector<V> v(n);
        const int kind = (int)(t % 4);
        std::normal_distribution<double> nd(0.0, 8.0);
        long nvis = 0;
        for (auto& x : v) {
            x = kind == 0 ? nd(rng) : kind == 1 ? std::round(nd(rng)) : kind == 2 ? (double)(rng() % 3) : nd(rng);
            if (kind == 3 && rng() % 5 == 0) x = DBL_MAX;
            nvis += x < DBL_MAX;
        }
        if (nvis == 0) { v[0] = 0.0; nvis = 1; }
        if (!check(v, kind == 3 ? nvis : 1 + (long)(rng() % (unsigned long)n), OW, MID, "random", false)) return 1;
    }
    std::printf("ok %ld %ld %ld\n", g_cases, g_mid, g_heap);
    return (g_mid > 0 && g_heap > 0) ? 0 : 2;
}
