// ct_settings_check.cpp -- a stand-alone host program around CtSettings, format_of() and reader() (csrc/container_internal.h),
// the rule behind glcPlanSetContainer* / glcPlanGetContainer*.  It is meant to be built with the host sanitizers and run on the
// CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/ct_settings_check.cpp -o ct_settings_check && ./ct_settings_check
// The rule used to be four mode booleans kept consistent by hand in every setter, four more derived from them by the encoder and
// a special case for the auto mode in format_of(); `Old` below restates it.  The program walks every state reachable from the
// default by setter calls (every setter with in-range, boundary and out-of-range values) on both rules in step and wants, for
// every call, the same return code, and in every state the same getter values, the same (version, flags, elem), the same reader
// mask, and the encoder's derived booleans equal to the settings' own.  It prints
//   ct_settings_check: ok, <states> states, <calls> calls
// That walk stays inside what the old rule knew: the codecs 0 and 1.  The CHOOSE codec (4) came later and has no older rule to
// be held against, so a second part states its rule outright and tries it from every state of the walk: accepted exactly with
// the shuffle off, it clears the mode, writes (3, 0, 0) and reads what a plain plan reads; while it is the codec every filter
// and every mode is refused with nothing changed, switching anything off is still accepted, and codec 0 or 1 leads back to
// that codec's plain state.  It prints
//   ct_settings_check: choose ok, <states> states
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"

#include <stdio.h>
#include <map>
#include <tuple>
#include <vector>

using namespace glc;

// the rule as it was: true = accepted
struct Old {
    uint32_t shuffle = 0; bool delta = false; uint32_t codec = 0; bool sparse = false, runs = false, ans = false, autom = false;
    bool set_shuffle(uint32_t elem)
    {
        if (elem > 1 && !(elem <= 8 && (CT_ELEMS >> elem & 1))) return false;
        shuffle = elem > 1 ? elem : 0;
        if (elem <= 1) delta = false;
        return true;
    }
    bool set_delta(uint32_t on)
    {
        if (on > 1 || (on && !shuffle)) return false;
        delta = on != 0;
        return true;
    }
    bool set_codec(uint32_t c)
    {
        if (c != CT_CODEC_BWT && c != CT_CODEC_HUFF0) return false;
        codec = c;
        if (c != CT_CODEC_HUFF0) sparse = ans = autom = false;
        if (c != CT_CODEC_BWT) runs = false;
        return true;
    }
    bool set_sparse(uint32_t on)
    {
        if (on > 1 || (on && (codec != CT_CODEC_HUFF0 || ans || autom))) return false;
        sparse = on != 0;
        return true;
    }
    bool set_ans(uint32_t on)
    {
        if (on > 1 || (on && (codec != CT_CODEC_HUFF0 || sparse || autom))) return false;
        ans = on != 0;
        return true;
    }
    bool set_auto(uint32_t on)
    {
        if (on > 1 || (on && (codec != CT_CODEC_HUFF0 || sparse || ans))) return false;
        autom = on != 0;
        return true;
    }
    bool set_runs(uint32_t on)
    {
        if (on > 1 || (on && codec != CT_CODEC_BWT)) return false;
        runs = on != 0;
        return true;
    }
    uint32_t reader() const
    {
        return (sparse ? CT_READS_SPARSE : 0u) | (runs ? CT_READS_RUNS : 0u) | (ans ? CT_READS_ANS : 0u) |
               (autom ? CT_READS_AUTO | CT_READS_SPARSE | CT_READS_ANS : 0u);
    }
    CtFormat format() const
    {
        CtFormat f;
        f.elem = shuffle;
        f.flags = shuffle && delta ? CT_FLAG_DELTA : 0;
        for (uint32_t i = 0; i < CT_NLEGAL; i++) {
            f.version = ct_legal(i).version;
            if (format_legal(f) && (codec != CT_CODEC_HUFF0 || f.kind2_legal()) && (!sparse || f.kind3_legal()) &&
                (!runs || f.kind4_legal()) && (!ans || f.kind5_legal()) && (!autom || f.version == CT_VERSION_AUTO)) break;
        }
        return f;
    }
    // what the encoder made of the settings
    bool enc_sparse() const { return sparse && codec == CT_CODEC_HUFF0; }
    bool enc_runs() const { return runs && codec == CT_CODEC_BWT; }
    bool enc_ans() const { return ans && codec == CT_CODEC_HUFF0 && !enc_sparse(); }
    bool enc_auto() const { return autom && codec == CT_CODEC_HUFF0 && !enc_sparse() && !enc_ans(); }
    auto key() const { return std::make_tuple(shuffle, delta, codec, sparse, runs, ans, autom); }
};

struct Both { Old o; CtSettings n; };

// setter k of 7 with value v on both rules: do they answer alike?
static bool call(Both &s, int k, uint32_t v)
{
    switch (k) {
    case 0: return s.o.set_shuffle(v) == s.n.set_shuffle(v);
    case 1: return s.o.set_delta(v) == s.n.set_delta(v);
    case 2: return s.o.set_codec(v) == s.n.set_codec(v);
    case 3: return s.o.set_sparse(v) == s.n.set_mode(CT_MODE_SPARSE, v);
    case 4: return s.o.set_runs(v) == s.n.set_mode(CT_MODE_RUNS, v);
    case 5: return s.o.set_ans(v) == s.n.set_mode(CT_MODE_ANS, v);
    default: return s.o.set_auto(v) == s.n.set_mode(CT_MODE_AUTO, v);
    }
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "ct_settings_check: line %d: %s\n", __LINE__, #x); return false; } } while (0)

static bool same_state(const Both &s)
{
    const Old &o = s.o;
    const CtSettings &n = s.n;
    CHECK(o.shuffle == n.shuffle && o.delta == n.delta && o.codec == n.codec);
    CHECK(o.sparse == (n.mode == CT_MODE_SPARSE) && o.runs == (n.mode == CT_MODE_RUNS) && o.ans == (n.mode == CT_MODE_ANS) &&
          o.autom == (n.mode == CT_MODE_AUTO));
    CHECK(o.enc_sparse() == o.sparse && o.enc_runs() == o.runs && o.enc_ans() == o.ans && o.enc_auto() == o.autom);
    CHECK(ct_mode_fits(n.mode, n.codec));
    const CtFormat fo = o.format(), fn = format_of(n);
    CHECK(fo.version == fn.version && fo.flags == fn.flags && fo.elem == fn.elem && format_legal(fn));
    CHECK(o.reader() == n.reader());
    return true;
}

int main()
{
    const std::vector<uint32_t> elems = {0, 1, 2, 3, 4, 8, 16, 255}, flags = {0, 1, 2, 0xFFFFFFFFu};
    std::vector<CtSettings> states;
    std::map<decltype(Old().key()), bool> seen;
    std::vector<Both> todo = {Both()};
    seen[todo[0].o.key()] = true;
    unsigned long long calls = 0;
    while (!todo.empty()) {
        const Both from = todo.back();
        todo.pop_back();
        if (!same_state(from)) return 1;
        states.push_back(from.n);
        for (int k = 0; k < 7; k++)
            for (uint32_t v : k == 0 ? elems : flags) {
                Both s = from;
                calls++;
                if (!call(s, k, v)) { fprintf(stderr, "ct_settings_check: setter %d with %u answers differently\n", k, v); return 1; }
                if (!same_state(s)) return 1;
                if (!seen[s.o.key()]) { seen[s.o.key()] = true; todo.push_back(s); }
            }
    }
    // the versions of the six (codec, mode) pairs without a filter
    const struct { uint32_t codec; CtMode mode; uint32_t version; } want[] = {
        {CT_CODEC_BWT, CT_MODE_PLAIN, CT_VERSION}, {CT_CODEC_BWT, CT_MODE_RUNS, CT_VERSION_RUNS}, {CT_CODEC_HUFF0, CT_MODE_PLAIN, CT_VERSION_CODEC},
        {CT_CODEC_HUFF0, CT_MODE_SPARSE, CT_VERSION_SPARSE}, {CT_CODEC_HUFF0, CT_MODE_ANS, CT_VERSION_ANS}, {CT_CODEC_HUFF0, CT_MODE_AUTO, CT_VERSION_AUTO}};
    for (const auto &w : want) {
        CtSettings n;
        if (!n.set_codec(w.codec) || !n.set_mode(w.mode, 1) || format_of(n).version != w.version) {
            fprintf(stderr, "ct_settings_check: codec %u mode %u does not write version %u\n", w.codec, (uint32_t)w.mode, w.version);
            return 1;
        }
    }
    printf("ct_settings_check: ok, %zu states, %llu calls\n", seen.size(), calls);
    const CtMode modes[] = {CT_MODE_SPARSE, CT_MODE_RUNS, CT_MODE_ANS, CT_MODE_AUTO};
    auto same = [](const CtSettings &a, const CtSettings &b) { return a.shuffle == b.shuffle && a.delta == b.delta && a.codec == b.codec && a.mode == b.mode; };
    auto choose_state = [&](const CtSettings &c) {
        CHECK(c.codec == CT_CODEC_CHOOSE && c.mode == CT_MODE_PLAIN && c.shuffle == 0 && !c.delta && c.reader() == 0);
        const CtFormat f = format_of(c);
        CHECK(f.version == CT_VERSION_CODEC && f.flags == 0 && f.elem == 0 && format_legal(f));
        CHECK(c.kinds() == (1u << CT_KIND_HUFF | 1u << CT_KIND_RAW | 1u << CT_KIND_HUFF0));
        return true;
    };
    for (const CtSettings &from : states) {
        CtSettings c = from;
        if (from.shuffle) {                                     // refused while the filter is on, nothing changed
            if (c.set_codec(CT_CODEC_CHOOSE) || !same(c, from)) { fprintf(stderr, "ct_settings_check: CHOOSE accepted with the shuffle on\n"); return 1; }
            continue;
        }
        if (!c.set_codec(CT_CODEC_CHOOSE) || !choose_state(c)) { fprintf(stderr, "ct_settings_check: CHOOSE refused or wrong with the shuffle off\n"); return 1; }
        const CtSettings at = c;
        for (uint32_t e : elems) {
            CtSettings t = at;
            const bool ok = t.set_shuffle(e);
            if (ok != (e <= 1) || !same(t, at)) { fprintf(stderr, "ct_settings_check: shuffle %u under CHOOSE\n", e); return 1; }
        }
        for (uint32_t v : flags) {
            CtSettings t = at;
            if (t.set_delta(v) != (v == 0) || !same(t, at)) { fprintf(stderr, "ct_settings_check: delta %u under CHOOSE\n", v); return 1; }
            for (CtMode m : modes) {
                t = at;
                if (t.set_mode(m, v) != (v == 0) || !same(t, at)) { fprintf(stderr, "ct_settings_check: mode %u = %u under CHOOSE\n", (uint32_t)m, v); return 1; }
            }
        }
        for (uint32_t k : {CT_CODEC_BWT, CT_CODEC_HUFF0, CT_CODEC_CHOOSE}) {
            CtSettings t = at, plain;
            plain.codec = k;
            if (!t.set_codec(k) || !same(t, plain)) { fprintf(stderr, "ct_settings_check: codec %u after CHOOSE\n", k); return 1; }
        }
        for (uint32_t k : {2u, 3u, 5u, 0xFFFFFFFFu}) {
            CtSettings t = at;
            if (t.set_codec(k) || !same(t, at)) { fprintf(stderr, "ct_settings_check: codec %u accepted\n", k); return 1; }
        }
    }
    printf("ct_settings_check: choose ok, %zu states\n", states.size());
    return 0;
}
