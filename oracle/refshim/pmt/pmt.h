/* Stand-in for <pmt/pmt.h> -- TEST INFRASTRUCTURE ONLY (oracle/refdriver.cc).  One tagged value type, enough to carry what the two
 * blocks publish and to let the driver read it back: symbols, blobs, integers, booleans, tuples, pairs, an empty dict, u8 vectors. */
#ifndef REFSHIM_PMT_PMT_H
#define REFSHIM_PMT_PMT_H
#include <gnuradio/types.h>

namespace pmt {

enum kind_t { PMT_SYMBOL, PMT_BLOB, PMT_LONG, PMT_UINT64, PMT_BOOL, PMT_TUPLE, PMT_PAIR, PMT_DICT, PMT_U8VECTOR };

struct pmt_base;
typedef boost::shared_ptr<pmt_base> pmt_t;

struct pmt_base {
    kind_t kind;
    std::string text;                  /* symbol */
    std::vector<unsigned char> bytes;  /* blob, u8vector */
    long long ival;                    /* long, bool */
    unsigned long long uval;           /* uint64 */
    std::vector<pmt_t> items;          /* tuple, pair (car, cdr) */
    explicit pmt_base(kind_t k) : kind(k), ival(0), uval(0) {}
};

static inline pmt_t make_kind(kind_t k) { return pmt_t(new pmt_base(k)); }

static inline pmt_t mp(const std::string &s) {
    pmt_t p = make_kind(PMT_SYMBOL);
    p->text = s;
    return p;
}
static inline pmt_t mp(const char *s) { return mp(std::string(s)); }
static inline pmt_t mp(const void *data, size_t len) {
    pmt_t p = make_kind(PMT_BLOB);
    const unsigned char *b = static_cast<const unsigned char *>(data);
    p->bytes.assign(b, b + len);
    return p;
}
static inline pmt_t from_long(long v) {
    pmt_t p = make_kind(PMT_LONG);
    p->ival = v;
    return p;
}
static inline pmt_t from_uint64(uint64_t v) {
    pmt_t p = make_kind(PMT_UINT64);
    p->uval = v;
    return p;
}
static inline pmt_t from_bool(bool v) {
    pmt_t p = make_kind(PMT_BOOL);
    p->ival = v ? 1 : 0;
    return p;
}
template <typename... T>
static inline pmt_t make_tuple(const T &... e) {
    pmt_t p = make_kind(PMT_TUPLE);
    p->items = std::vector<pmt_t>{e...};
    return p;
}
static inline pmt_t cons(const pmt_t &car, const pmt_t &cdr) {
    pmt_t p = make_kind(PMT_PAIR);
    p->items.push_back(car);
    p->items.push_back(cdr);
    return p;
}
static inline pmt_t make_dict() { return make_kind(PMT_DICT); }
static inline pmt_t init_u8vector(size_t n, const uint8_t *data) {
    pmt_t p = make_kind(PMT_U8VECTOR);
    p->bytes.assign(data, data + n);
    return p;
}
static inline bool is_blob(const pmt_t &p) { return p && p->kind == PMT_BLOB; }
static inline size_t blob_length(const pmt_t &p) { return p->bytes.size(); }
static inline const void *blob_data(const pmt_t &p) { return p->bytes.data(); }

}  // namespace pmt

#endif
