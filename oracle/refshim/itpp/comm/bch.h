/* Stand-in for <itpp/comm/bch.h> -- TEST INFRASTRUCTURE ONLY (oracle/refdriver.cc).
 *
 * bvec: a vector of bits, one byte each.  operator[] tolerates an index beyond the size (it hands out a scratch element): the caller
 * this stands in for reads entries 36..47 of a 36-element vector and never uses what it read.
 *
 * BCH(63, 2, true)::decode is a BRUTE-FORCE TABLE decoder, written for this file alone (it includes, links and calls nothing of
 * oracle/ref_chain.c, and tests/bchref.py is what it is held to, on all 4096 syndromes): the remainder of the received word modulo
 * the generator x^12 + x^10 + x^8 + x^5 + x^4 + x^3 + 1 indexes a table of error patterns that is filled at construction by enumerating
 * every pattern of weight 0, 1 and 2 (2017 remainders; d_min = 5 keeps them apart), and then the 21 patterns x^k + x^(k+21) + x^(k+42),
 * k = 0..20: the documented IT++ rule -- the decoder accepts a word whose locator has as many roots as its degree, and for S1 = 0 with
 * S3 a cube those are these three positions -- so such a word is "corrected" at weight 3 and reported valid.  Entry j of a word is the
 * coefficient of x^(62-j); systematic: the message is entries 0..50.  A word whose remainder is not in the table is reported invalid and
 * its message entries are returned as received.  This is a stand-in for the VERDICT only; IT++ itself stays unpinned. */
#ifndef REFSHIM_ITPP_COMM_BCH_H
#define REFSHIM_ITPP_COMM_BCH_H
#include <stdint.h>
#include <iostream>
#include <vector>

namespace itpp {

class bvec {
public:
    bvec() : d_scratch(0) {}
    explicit bvec(int n) : d_bits(n > 0 ? n : 0, 0), d_scratch(0) {}
    bvec(const char *text) : d_scratch(0) {
        for (const char *p = text; *p; p++)
            if (*p == '0' || *p == '1') d_bits.push_back(*p - '0');
    }
    int size() const { return (int)d_bits.size(); }
    int length() const { return size(); }
    void set_size(int n) { d_bits.assign(n > 0 ? n : 0, 0); }
    unsigned char &operator[](int i) {
        if (i < 0 || i >= size()) {
            d_scratch = 0;
            return d_scratch;
        }
        return d_bits[i];
    }
    unsigned char operator[](int i) const { return (i < 0 || i >= size()) ? 0 : d_bits[i]; }
    /* entries first..last, both included */
    bvec operator()(int first, int last) const {
        bvec out;
        for (int i = first; i <= last && i < size(); i++)
            if (i >= 0) out.d_bits.push_back(d_bits[i]);
        return out;
    }
    void push_back(unsigned char b) { d_bits.push_back(b & 1); }

private:
    std::vector<unsigned char> d_bits;
    unsigned char d_scratch;
};

inline bvec concat(const bvec &a, const bvec &b) {
    bvec out;
    for (int i = 0; i < a.size(); i++) out.push_back(a[i]);
    for (int i = 0; i < b.size(); i++) out.push_back(b[i]);
    return out;
}

inline std::ostream &operator<<(std::ostream &os, const bvec &v) {
    os << "[";
    for (int i = 0; i < v.size(); i++) os << (i ? " " : "") << (int)v[i];
    return os << "]";
}

class BCH {
public:
    enum { N = 63, K = 51, NSYN = 4096 };
    static const uint32_t GENERATOR = 0x1539; /* 1 0101 0011 1001 */

    BCH(int n, int t, bool systematic) : d_table(NSYN, NO_PATTERN) {
        d_usable = (n == N && t == 2 && systematic);
        enter(0);
        for (int i = 0; i < N; i++) enter(1ull << i);
        for (int i = 0; i < N; i++)
            for (int j = 0; j < i; j++) enter((1ull << i) | (1ull << j));
        for (int k = 0; k < 21; k++) enter((1ull << k) | (1ull << (k + 21)) | (1ull << (k + 42)));
    }

    static uint32_t remainder(uint64_t word) {
        for (int d = N - 1; d >= 12; d--)
            if ((word >> d) & 1) word ^= (uint64_t)GENERATOR << (d - 12);
        return (uint32_t)word;
    }

    /* the table itself, for the driver's `bch` mode: the error pattern for a remainder (bit e = x^e), or NO_PATTERN */
    enum : uint64_t { NO_PATTERN = ~0ull };
    uint64_t pattern(uint32_t rem) const { return d_table[rem & (NSYN - 1)]; }

    bool decode(const bvec &coded, bvec &decoded, bvec &cw_isvalid) {
        const int blocks = coded.size() / N;
        bool all = true;
        decoded.set_size(blocks * K);
        cw_isvalid.set_size(blocks);
        for (int b = 0; b < blocks; b++) {
            uint64_t word = 0;
            for (int j = 0; j < N; j++) word |= (uint64_t)(coded[b * N + j] & 1) << (N - 1 - j);
            const uint64_t err = d_usable ? d_table[remainder(word)] : NO_PATTERN;
            const bool ok = err != NO_PATTERN;
            if (ok) word ^= err;
            for (int j = 0; j < K; j++) decoded[b * K + j] = (word >> (N - 1 - j)) & 1;
            cw_isvalid[b] = ok;
            all = all && ok;
        }
        return all;
    }

private:
    void enter(uint64_t pattern) {
        const uint32_t r = remainder(pattern);
        if (d_table[r] == NO_PATTERN) d_table[r] = pattern;
    }
    std::vector<uint64_t> d_table;
    bool d_usable;
};

}  // namespace itpp

#endif
