/* oracle/refdriver.cc -- TEST INFRASTRUCTURE ONLY.  A stand-alone program that pushes committed inputs through the REFERENCE'S OWN
 * object code (recc_impl.cc, recc_decode_impl.cc, amps_packet.cc, utils.cc compiled in place against the stand-in headers of
 * oracle/refshim/, recipe: oracle/Makefile, target _ref) and writes down what comes out.  The reference's headers are included by
 * name; nothing of the reference's text is in this file.  It is built only where the reference's sources are present and is never
 * committed; tests/golden/make_reference_compiled.py runs it and keeps its inputs and outputs as a fixture.
 *
 *   refdriver work   IN OUT   symbol streams with a chunk schedule through recc_impl::work
 *   refdriver decode IN OUT   3374-byte bursts through the handler recc_decode_impl registered for "bursts"
 *   refdriver fields IN OUT   words and values through the parsers, the MIN arithmetic, the FOCC/FVC word builders, the Manchester
 *                             decoder, and the trigger the recc constructor builds
 *   refdriver bch    IN OUT   63-bit words through the stand-in itpp::BCH(63,2,true) (the stand-in's own verdict: see refshim/itpp)
 *
 * File formats (all integers little endian):
 *   work   IN : per stream  u32 nsym, u32 ncalls, u32 size[ncalls], u8 sym[nsym]          (sum of sizes = nsym)
 *          OUT: per publish u32 stream, u32 call, u8 payload[3374]
 *   decode IN : u8 burst[3374] per burst;   OUT: text, see decode_mode()
 *   fields IN : u8 tag + payload per record; OUT: text, one line per record, see fields_mode()
 *   bch    IN : u8 bit[63] per word;        OUT: text "BCH <ok> <51 message bits> <error pattern, hex, bit e = x^e, or ->"
 *
 * The reference prints on every call (and says which branch it took only there), so stdout is redirected into a temporary file around
 * every call and read back.  Its log lines are recognised by the source file and LINE NUMBER they carry; only values derived from
 * them are written out: class, MIN, ESN, dialled digits and two warnings -- no path, no time stamp, no text.
 * The reference asserts what it needs of its input and is built with its default -DNDEBUG, so the driver checks instead: every symbol
 * is 0 or 1, a work() call is shorter than 61 440 symbols. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <iostream>
#include <string>
#include <vector>

#include "recc_impl.h"
#include "recc_decode_impl.h"
#include "amps_packet.h"
#include "utils.h"

namespace {

const size_t CAPTURE = 3374;
const int MAX_WORK = 65536 - 4096; /* a call must be shorter than this */

void die(const char *what) {
    fprintf(stderr, "refdriver: %s\n", what);
    exit(2);
}

/* ------------------------------------------------------------------ stdout capture */
int g_saved_stdout = -1;
FILE *g_capture = NULL;

void capture_begin() {
    fflush(stdout);
    std::cout.flush();
    g_capture = tmpfile();
    if (!g_capture) die("tmpfile failed");
    g_saved_stdout = dup(1);
    if (g_saved_stdout < 0 || dup2(fileno(g_capture), 1) < 0) die("cannot redirect stdout");
}

std::string capture_end() {
    fflush(stdout);
    std::cout.flush();
    if (dup2(g_saved_stdout, 1) < 0) die("cannot restore stdout");
    close(g_saved_stdout);
    std::string text;
    char buf[4096];
    size_t n;
    rewind(g_capture);
    while ((n = fread(buf, 1, sizeof buf, g_capture)) > 0) text.append(buf, n);
    fclose(g_capture);
    g_capture = NULL;
    return text;
}

/* one LOG_DEBUG / LOG_WARNING line: "<stamp>: <file>:<line> <LEVEL>: <text>" */
struct LogLine {
    std::string file; /* base name */
    int line;
    std::string text;
};

std::vector<LogLine> log_lines(const std::string &captured) {
    std::vector<LogLine> out;
    size_t at = 0;
    while (at < captured.size()) {
        size_t end = captured.find('\n', at);
        if (end == std::string::npos) end = captured.size();
        const std::string ln = captured.substr(at, end - at);
        at = end + 1;
        size_t mark = ln.find(" DEBUG: "), skip = 8;
        if (mark == std::string::npos) {
            mark = ln.find(" WARNING: ");
            skip = 10;
        }
        if (mark == std::string::npos) continue;
        const std::string head = ln.substr(0, mark);
        const size_t colon = head.rfind(':');
        if (colon == std::string::npos || colon + 1 >= head.size()) continue;
        LogLine l;
        l.line = atoi(head.c_str() + colon + 1);
        std::string path = head.substr(0, colon);
        const size_t cut = path.find_last_of("/ ");
        l.file = cut == std::string::npos ? path : path.substr(cut + 1);
        l.text = ln.substr(mark + skip);
        out.push_back(l);
    }
    return out;
}

/* the token behind `key` up to the next blank (or the rest of the line with rest = true); "" when the key is absent */
std::string value_of(const std::string &text, const char *key, bool rest = false) {
    const size_t at = text.find(key);
    if (at == std::string::npos) return "";
    const size_t from = at + strlen(key);
    if (rest) return text.substr(from);
    const size_t to = text.find(' ', from);
    return text.substr(from, to == std::string::npos ? std::string::npos : to - from);
}

/* ------------------------------------------------------------------ small helpers */
std::vector<unsigned char> read_all(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) die("cannot open the input file");
    std::vector<unsigned char> data;
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
    fclose(f);
    return data;
}

struct Reader {
    const std::vector<unsigned char> &d;
    size_t at;
    explicit Reader(const std::vector<unsigned char> &data) : d(data), at(0) {}
    bool done() const { return at >= d.size(); }
    const unsigned char *take(size_t n) {
        if (n > d.size() - at) die("input file ends inside a record");
        const unsigned char *p = &d[at];
        at += n;
        return p;
    }
    uint64_t uint(int bytes) {
        const unsigned char *p = take(bytes);
        uint64_t v = 0;
        for (int i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i);
        return v;
    }
};

void require_binary(const unsigned char *p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (p[i] > 1) die("input holds a symbol that is neither 0 nor 1");
}

std::string bit_string(const unsigned char *p, size_t n) {
    std::string s(n, '0');
    for (size_t i = 0; i < n; i++) s[i] = p[i] ? '1' : '0';
    return s;
}

void put_u32(FILE *f, uint32_t v) {
    unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
    fwrite(b, 1, 4, f);
}

/* ------------------------------------------------------------------ work */
int work_mode(Reader &in, FILE *out) {
    for (uint32_t stream = 0; !in.done(); stream++) {
        const uint32_t nsym = (uint32_t)in.uint(4), ncalls = (uint32_t)in.uint(4);
        std::vector<uint32_t> sizes(ncalls);
        uint64_t total = 0;
        for (uint32_t i = 0; i < ncalls; i++) {
            sizes[i] = (uint32_t)in.uint(4);
            if (sizes[i] < 1 || sizes[i] >= (uint32_t)MAX_WORK) die("a work() call of no symbol, or of 61 440 or more");
            total += sizes[i];
        }
        if (total != nsym) die("the schedule does not add up to the stream");
        const unsigned char *sym = in.take(nsym);
        require_binary(sym, nsym);
        gr::amps::recc::sptr block = gr::amps::recc::make();
        gr_vector_const_void_star ins(1);
        gr_vector_void_star outs;
        size_t off = 0;
        capture_begin();
        for (uint32_t call = 0; call < ncalls; call++) {
            ins[0] = sym + off;
            block->published.clear();
            block->work((int)sizes[call], ins, outs);
            off += sizes[call];
            for (size_t k = 0; k < block->published.size(); k++) {
                const pmt::pmt_t &msg = block->published[k].second;
                if (block->published[k].first != "bursts" || !pmt::is_blob(msg) || pmt::blob_length(msg) != CAPTURE)
                    die("recc published something that is not a 3374-byte blob on \"bursts\"");
                put_u32(out, stream);
                put_u32(out, call);
                fwrite(pmt::blob_data(msg), 1, CAPTURE, out);
            }
        }
        capture_end();
    }
    return 0;
}

/* ------------------------------------------------------------------ decode */
enum { CLS_INVALID_WORD_A, CLS_E_ZERO, CLS_PAGE_RESPONSE, CLS_REGISTRATION, CLS_ORIGINATION, CLS_BAD_NAWC, CLS_UNKNOWN };

void print_a(FILE *out, const gr::amps::recc_word_a &a) {
    fprintf(out, "A F=%d NAWC=%d T=%d S=%d E=%d ER=%d SCM=%d MIN1=%llu\n", (int)a.F, (int)a.NAWC, (int)a.T, (int)a.S, (int)a.E, (int)a.ER,
            (int)a.SCM, (unsigned long long)a.MIN1);
}

void print_b(FILE *out, const gr::amps::recc_word_b &b) {
    fprintf(out, "B F=%d NAWC=%d MSG_TYPE=%d ORDQ=%d ORDER=%d LT=%d EP=%d SCM4=%d MPCI=%d SDCC1=%d SDCC2=%d MIN2=%llu\n", (int)b.F, (int)b.NAWC,
            (int)b.MSG_TYPE, (int)b.ORDQ, (int)b.ORDER, (int)b.LT, (int)b.EP, (int)b.SCM4, (int)b.MPCI, (int)b.SDCC1, (int)b.SDCC2,
            (unsigned long long)b.MIN2);
}

void print_message(FILE *out, const std::string &port, const pmt::pmt_t &m) {
    using namespace pmt;
    if (port == "focc_words" && m->kind == PMT_TUPLE && m->items.size() == 4) {
        fprintf(out, "MSG focc_words stream=%lld n=%lld w1=%s w2=%s\n", m->items[0]->ival, m->items[1]->ival,
                bit_string(m->items[2]->bytes.data(), m->items[2]->bytes.size()).c_str(),
                bit_string(m->items[3]->bytes.data(), m->items[3]->bytes.size()).c_str());
    } else if (port == "fvc_words" && m->kind == PMT_TUPLE && m->items.size() == 3) {
        fprintf(out, "MSG fvc_words n=%lld w1=%s repeat=%llu\n", m->items[0]->ival,
                bit_string(m->items[1]->bytes.data(), m->items[1]->bytes.size()).c_str(), m->items[2]->uval);
    } else if ((port == "fvc_mute" || port == "audio_mute") && m->kind == PMT_BOOL) {
        fprintf(out, "MSG %s %lld\n", port.c_str(), m->ival);
    } else if (port == "command_out" && m->kind == PMT_PAIR && m->items[1]->kind == PMT_U8VECTOR) {
        fprintf(out, "MSG command_out %s\n", std::string(m->items[1]->bytes.begin(), m->items[1]->bytes.end()).c_str());
    } else {
        die("recc_decode published a message of a shape the driver does not know");
    }
}

/* per burst:  BURST <i> / CLASS <0..6> / [MIN <10 digits>] / [ESN <hex>] / [DIALED <digits>] / [FLAG nawc_mismatch] / [FLAG bad_digit] /
 * DCC <7 bits> <bad pairs> / MANCH <bad pairs of the seven words> / A ... / B ... / MSG ... / END.
 * DCC, MANCH, A and B come from the reference's Manchester decoder and word parsers applied the way bursts_message applies them (to
 * the symbols behind the DCC, to repeat 0 of words 0 and 1 as received). */
int decode_mode(Reader &in, FILE *out) {
    gr::amps::recc_decode::sptr block = gr::amps::recc_decode::make();
    if (!block->handlers.count("bursts")) die("recc_decode registered no handler for \"bursts\"");
    for (int i = 0; !in.done(); i++) {
        const unsigned char *burst = in.take(CAPTURE);
        require_binary(burst, CAPTURE);
        block->published.clear();
        capture_begin();
        block->handlers["bursts"](pmt::mp(burst, CAPTURE));
        unsigned char dcc[7], words[7][240];
        size_t manch[7];
        const size_t dcc_bad = gr::amps::manchester_decode_binbuf(burst, dcc, 7);
        for (int w = 0; w < 7; w++) manch[w] = gr::amps::manchester_decode_binbuf(burst + 14 + 480 * w, words[w], 240);
        const gr::amps::recc_word_a a(words[0]);
        const gr::amps::recc_word_b b(words[1]);
        const std::vector<LogLine> log = log_lines(capture_end());

        int cls = -1;
        bool nawc_mismatch = false, bad_digit = false, has_esn_line = false;
        std::string min, esn, dialed;
        for (size_t k = 0; k < log.size(); k++) {
            const LogLine &l = log[k];
            if (l.file == "amps_packet.h" && l.line == 222) {
                bad_digit = true;
            } else if (l.file == "recc_decode_impl.cc") {
                switch (l.line) {
                    case 109: cls = CLS_INVALID_WORD_A; break;
                    case 114: cls = CLS_E_ZERO; break;
                    case 200: cls = CLS_PAGE_RESPONSE; min = value_of(l.text, "MIN="); break;
                    case 126: cls = CLS_REGISTRATION; min = value_of(l.text, "MIN="); break;
                    case 132: esn = value_of(l.text, "ESN="); has_esn_line = true; break;
                    case 135: case 151: nawc_mismatch = true; break;
                    case 156: cls = CLS_BAD_NAWC; break;
                    case 182: break; /* the registration's reply is announced; the class was set at 126 */
                    case 238:
                        cls = CLS_ORIGINATION;
                        min = value_of(l.text, "MIN=");
                        esn = value_of(l.text, "ESN=");
                        has_esn_line = true;
                        dialed = value_of(l.text, "dialed ", true);
                        break;
                    case 167: cls = CLS_UNKNOWN; break;
                    default: die("a log line of recc_decode_impl.cc at a line number the driver does not know");
                }
            }
        }
        if (cls < 0) die("the reference took a branch that logs nothing");
        fprintf(out, "BURST %d\nCLASS %d\n", i, cls);
        if (!min.empty()) fprintf(out, "MIN %s\n", min.c_str());
        if (has_esn_line) fprintf(out, "ESN %s\n", esn.c_str());
        if (cls == CLS_ORIGINATION) fprintf(out, "DIALED %s\n", dialed.c_str());
        if (nawc_mismatch) fprintf(out, "FLAG nawc_mismatch\n");
        if (bad_digit) fprintf(out, "FLAG bad_digit\n");
        fprintf(out, "DCC %s %zu\n", bit_string(dcc, 7).c_str(), dcc_bad);
        fprintf(out, "MANCH %zu %zu %zu %zu %zu %zu %zu\n", manch[0], manch[1], manch[2], manch[3], manch[4], manch[5], manch[6]);
        print_a(out, a);
        print_b(out, b);
        for (size_t k = 0; k < block->published.size(); k++) print_message(out, block->published[k].first, block->published[k].second);
        fprintf(out, "END\n");
    }
    return 0;
}

/* ------------------------------------------------------------------ fields */
enum {
    TAG_WORD_A = 1,      /* u8 bit[48]                              -> A ... */
    TAG_WORD_B = 2,      /* u8 bit[48]                              -> B ... */
    TAG_WORD_C = 3,      /* u8 bit[48]                              -> C F= NAWC= SERIAL= */
    TAG_WORD_CALLED = 4, /* u8 bit[48]                              -> D F= NAWC= DIGITS= digits=<s> bad=<0|1> */
    TAG_EXTRACT_ALL = 5, /* (nothing)                               -> 1024 lines X3 <value> <three digits> */
    TAG_PARSE_MIN = 6,   /* u8 digit[10] (ASCII)                    -> PM <ok> <MIN1> <MIN2> <calc_min of them> */
    TAG_CALC_MIN = 7,    /* u64 MIN1, u64 MIN2                      -> CM <ten digits> */
    TAG_FOCC_WORD1 = 8,  /* u8 multiword, u8 dcc, u64 MIN1          -> W <28 bits> */
    TAG_FOCC_WORD2_GENERAL = 9,        /* u64 MIN2, u8 msg_type, u8 ordq, u8 order     -> W */
    TAG_FOCC_WORD2_VOICE_CHANNEL = 10, /* u8 scc, u64 MIN2, u8 vmac, u16 chan          -> W */
    TAG_FVC_WORD1_GENERAL = 11,        /* u8 pscc, u8 msg_type, u8 ordq, u8 order      -> W */
    TAG_MANCHESTER = 12, /* u32 nbits, u8 sym[2 nbits]              -> MD <bits> <bad pairs> */
    TAG_TRIGGER = 13     /* (nothing)                               -> TRIG <the symbols the recc constructor built> */
};

int fields_mode(Reader &in, FILE *out) {
    using namespace gr::amps;
    while (!in.done()) {
        const int tag = (int)in.uint(1);
        unsigned char word[48] = {0}, w28[28];
        if (tag >= TAG_WORD_A && tag <= TAG_WORD_CALLED) {
            const unsigned char *p = in.take(48);
            require_binary(p, 48);
            memcpy(word, p, 48);
        }
        capture_begin();
        std::string digits;
        recc_word_called called(word); /* read below only under its own tag */
        switch (tag) {
            case TAG_WORD_CALLED: digits = called.digits(); break;
            default: break;
        }
        const std::vector<LogLine> log = log_lines(capture_end());
        switch (tag) {
            case TAG_WORD_A: print_a(out, recc_word_a(word)); break;
            case TAG_WORD_B: print_b(out, recc_word_b(word)); break;
            case TAG_WORD_C: {
                const recc_word_c_serial c(word);
                fprintf(out, "C F=%d NAWC=%d SERIAL=%lu\n", (int)c.F, (int)c.NAWC, c.SERIAL);
                break;
            }
            case TAG_WORD_CALLED: {
                bool bad = false;
                for (size_t k = 0; k < log.size(); k++) bad = bad || (log[k].file == "amps_packet.h" && log[k].line == 222);
                fprintf(out, "D F=%d NAWC=%d DIGITS=%lu digits=%s bad=%d\n", (int)called.F, (int)called.NAWC, called.DIGITS, digits.c_str(), (int)bad);
                break;
            }
            case TAG_EXTRACT_ALL:
                for (unsigned v = 0; v < 1024; v++) fprintf(out, "X3 %u %s\n", v, extract_min_3(v).c_str());
                break;
            case TAG_PARSE_MIN: {
                const unsigned char *p = in.take(10);
                for (int i = 0; i < 10; i++)
                    if (p[i] < '0' || p[i] > '9') die("a MIN string needs ten digits");
                u_int64_t min1 = 0, min2 = 0;
                const bool ok = parse_min(std::string((const char *)p, 10), min1, min2);
                fprintf(out, "PM %d %llu %llu %s\n", (int)ok, (unsigned long long)min1, (unsigned long long)min2, calc_min(min1, min2).c_str());
                break;
            }
            case TAG_CALC_MIN: {
                const u_int64_t min1 = in.uint(8), min2 = in.uint(8);
                fprintf(out, "CM %s\n", calc_min(min1, min2).c_str());
                break;
            }
            case TAG_FOCC_WORD1: {
                const int multi = (int)in.uint(1), dcc = (int)in.uint(1);
                focc_word1(w28, multi != 0, (unsigned char)dcc, in.uint(8));
                fprintf(out, "W %s\n", bit_string(w28, 28).c_str());
                break;
            }
            case TAG_FOCC_WORD2_GENERAL: {
                const u_int64_t min2 = in.uint(8);
                const int t = (int)in.uint(1), q = (int)in.uint(1), o = (int)in.uint(1);
                focc_word2_general(w28, min2, (unsigned char)t, (unsigned char)q, (unsigned char)o);
                fprintf(out, "W %s\n", bit_string(w28, 28).c_str());
                break;
            }
            case TAG_FOCC_WORD2_VOICE_CHANNEL: {
                const int scc = (int)in.uint(1);
                const u_int64_t min2 = in.uint(8);
                const int vmac = (int)in.uint(1), chan = (int)in.uint(2);
                focc_word2_voice_channel(w28, (unsigned char)scc, min2, (unsigned char)vmac, (unsigned short)chan);
                fprintf(out, "W %s\n", bit_string(w28, 28).c_str());
                break;
            }
            case TAG_FVC_WORD1_GENERAL: {
                const int pscc = (int)in.uint(1), t = (int)in.uint(1), q = (int)in.uint(1), o = (int)in.uint(1);
                fvc_word1_general(w28, (unsigned char)pscc, (unsigned char)t, (unsigned char)q, (unsigned char)o);
                fprintf(out, "W %s\n", bit_string(w28, 28).c_str());
                break;
            }
            case TAG_MANCHESTER: {
                const size_t nbits = (size_t)in.uint(4);
                if (nbits < 1) die("a Manchester record of no bit");
                const unsigned char *sym = in.take(2 * nbits);
                require_binary(sym, 2 * nbits);
                std::vector<unsigned char> bits(nbits);
                const size_t bad = manchester_decode_binbuf(sym, bits.data(), nbits);
                fprintf(out, "MD %s %zu\n", bit_string(bits.data(), nbits).c_str(), bad);
                break;
            }
            case TAG_TRIGGER: {
                recc::sptr block = recc::make();
                /* the trigger is private to recc_impl: this file alone is compiled with -fno-access-control */
                const recc_impl *impl = dynamic_cast<const recc_impl *>(block.get());
                if (!impl) die("recc::make() did not return a recc_impl");
                fprintf(out, "TRIG %s\n", bit_string(impl->trigger_data, impl->trigger_len).c_str());
                break;
            }
            default: die("unknown record tag in a fields file");
        }
    }
    return 0;
}

/* ------------------------------------------------------------------ bch */
int bch_mode(Reader &in, FILE *out) {
    itpp::BCH bch(63, 2, true);
    while (!in.done()) {
        const unsigned char *p = in.take(63);
        require_binary(p, 63);
        itpp::bvec coded(63), decoded, valid;
        uint64_t word = 0;
        for (int j = 0; j < 63; j++) {
            coded[j] = p[j];
            word |= (uint64_t)p[j] << (62 - j);
        }
        const bool ok = bch.decode(coded, decoded, valid);
        unsigned char msg[51];
        for (int j = 0; j < 51; j++) msg[j] = decoded[j];
        const uint64_t err = bch.pattern(itpp::BCH::remainder(word));
        if (ok)
            fprintf(out, "BCH 1 %s %llx\n", bit_string(msg, 51).c_str(), (unsigned long long)err);
        else
            fprintf(out, "BCH 0 %s -\n", bit_string(msg, 51).c_str());
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: refdriver work|decode|fields|bch IN OUT\n");
        return 2;
    }
    const std::vector<unsigned char> data = read_all(argv[2]);
    Reader in(data);
    FILE *out = fopen(argv[3], "wb");
    if (!out) die("cannot open the output file");
    const std::string mode = argv[1];
    int rc = 2;
    if (mode == "work")
        rc = work_mode(in, out);
    else if (mode == "decode")
        rc = decode_mode(in, out);
    else if (mode == "fields")
        rc = fields_mode(in, out);
    else if (mode == "bch")
        rc = bch_mode(in, out);
    else
        die("unknown mode");
    if (fclose(out) != 0) die("cannot write the output file");
    return rc;
}
