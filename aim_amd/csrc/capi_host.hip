// capi_host.hip -- the host-side helpers of the C-ABI (include/aim_hip.h): the launchers' size rule, CIGAR formatting, sequence packing
// and the pair generator. No HIP call and no kernel here; what this unit shares with aim_capi.hip is in capi_common.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "capi_common.hpp"
#include "batch_io.hpp"   // packed_row_dwords

using namespace aim::capi;

// aim_cigar_format and aim_cigar_format_runs: "<length><op>" for every maximal run of equal ops over n >= 1 items, item i being
// len_of(i) times op_of(i), then a newline. Returns the characters written.
template <typename Op, typename Len>
static int cigar_line(uint32_t n, Op op_of, Len len_of, char *out, int32_t cap)
{
    int at = 0;
    char last_op = op_of(0);
    uint32_t run = len_of(0);
    for (uint32_t i = 1; i < n; ++i) {
        const char op = op_of(i);
        if (op == last_op) {
            run += len_of(i);
        } else {
            at += snprintf(out + at, (size_t)(cap - at), "%u%c", run, last_op);
            if (at >= cap - 1) return fail(AIM_EINVAL, "cigar buffer too small");
            last_op = op;
            run = len_of(i);
        }
    }
    at += snprintf(out + at, (size_t)(cap - at), "%u%c\n", run, last_op);
    if (at >= cap) return fail(AIM_EINVAL, "cigar buffer too small");
    return at;
}

extern "C" {

int aim_launcher_sizes(int32_t algo, int32_t read_length, double error, int32_t mismatch, int32_t gap_o,
                       int32_t gap_e, int32_t gap, int32_t *max_score, int32_t *read_size)
{
    if (!max_score || !read_size || read_length <= 0) return fail(AIM_EINVAL, "bad arguments");
    // Python float arithmetic of the launchers == IEEE double here.
    volatile double wrong = (double)read_length * error;
    volatile double a = wrong * (double)mismatch;
    volatile double b = (algo == AIM_ALGO_NW) ? wrong * (double)gap : wrong * (double)(gap_o + gap_e);
    *max_score = (int32_t)std::ceil(a > b ? a : b);
    volatile double t = (double)read_length + wrong;
    t = t + 7.0;
    t = t / 8.0;
    *read_size = (int32_t)std::ceil(t) * 8;
    return AIM_OK;
}

int aim_cigar_format(const char *ops, int32_t begin_offset, int32_t end_offset, char *out, int32_t cap)
{
    if (!ops || !out || cap < 4 || begin_offset < 0) return fail(AIM_EINVAL, "bad arguments");
    const uint32_t n = end_offset > begin_offset ? (uint32_t)(end_offset - begin_offset) : 1u;   // (ops[begin_offset] is read in any case)
    return cigar_line(n, [&](uint32_t i) { return ops[begin_offset + i]; }, [](uint32_t) { return 1u; }, out, cap);
}

int aim_sam_format_cigar(const uint32_t *words, uint32_t n, char *out, int32_t cap)
{
    if (!out || cap < 2 || (n && !words)) return fail(AIM_EINVAL, "aim_sam_format_cigar: bad arguments");
    if (!n) { out[0] = '*'; out[1] = 0; return 1; }
    int at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t op = words[i] & 0xfu;
        if (op > 8u) return fail(AIM_EINVAL, "aim_sam_format_cigar: word %u holds op %u", i, op);
        const int w = snprintf(out + at, (size_t)(cap - at), "%u%c", words[i] >> 4, "MIDNSHP=X"[op]);
        if (w < 0 || w >= cap - at) return fail(AIM_EINVAL, "aim_sam_format_cigar: output buffer too small");
        at += w;
    }
    return at;
}

int aim_pack_sequence(const char *seq, int32_t len, int32_t read_size, uint32_t *row)
{
    if (!seq || !row || len < 0 || len > read_size) return fail(AIM_EINVAL, "bad arguments");
    const uint32_t dw = aim::packed_row_dwords(read_size);
    uint32_t bad = 0;
    int i = 0;
    for (uint32_t w = 0; w < dw; ++w) {
        uint32_t v = 0;
        const int lim = std::min(len, (int)(w + 1) * 16);
        for (int sh = 0; i < lim; ++i, sh += 2) {
            const unsigned char c = (unsigned char)seq[i];
            const uint32_t code = (c >> 1) & 3u;
            bad |= (uint32_t)(c ^ (unsigned char)"ACTG"[code]);
            v |= code << sh;
        }
        row[w] = v;
    }
    return bad == 0;
}

int aim_pack_batch(const aim_params_t *params, uint32_t n_pairs, const void *requests, const char *patterns, const char *texts,
                   uint32_t *packed_patterns, uint32_t *packed_texts, uint32_t *raw_pairs, char *raw_patterns, char *raw_texts,
                   uint32_t max_raw, uint32_t *n_raw, int threads)
{
    // AIM_FLAG_REF_TEXTS: the texts are windows of the device's reference; only the patterns are packed (texts / packed_texts may be NULL)
    const bool ref = params && is_ref(*params);
    if (!params || !n_raw || (n_pairs && (!requests || !patterns || !packed_patterns || (!ref && (!texts || !packed_texts)))))
        return fail(AIM_EINVAL, "bad arguments");
    const int rs = params->read_size;
    if (rs <= 0 || (rs & 7)) return fail(AIM_EINVAL, "read_size must be a positive multiple of 8");
    int rc = check_lengths(*params, n_pairs, requests);
    if (rc) return rc;
    const uint32_t dw = aim::packed_row_dwords(rs);
    const bool req8 = params->flags & AIM_FLAG_REQ8;
    if (threads < 1) threads = 1;
    if (threads > 256) threads = 256;
    std::vector<uint8_t> is_raw(n_pairs, 0);
    auto work = [&](int t) {
        const size_t lo = (size_t)n_pairs * t / threads, hi = (size_t)n_pairs * (t + 1) / threads;
        for (size_t i = lo; i < hi; ++i) {
            const int pl = req8 ? static_cast<const aim_request8_t *>(requests)[i].pattern_len : static_cast<const aim_request_t *>(requests)[i].pattern_len;
            const int tl = req8 ? static_cast<const aim_request8_t *>(requests)[i].text_len : static_cast<const aim_request_t *>(requests)[i].text_len;
            const int okp = aim_pack_sequence(patterns + i * rs, pl, rs, packed_patterns + i * dw);
            const int okt = (texts && packed_texts) ? aim_pack_sequence(texts + i * rs, tl, rs, packed_texts + i * dw) : 1;
            is_raw[i] = !(okp == 1 && okt == 1);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < threads; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_pairs; ++i) {
        if (!is_raw[i]) continue;
        if (n < max_raw && raw_pairs && raw_patterns && (raw_texts || !texts)) {
            raw_pairs[n] = i;
            memcpy(raw_patterns + (size_t)n * rs, patterns + (size_t)i * rs, (size_t)rs);
            if (raw_texts && texts) memcpy(raw_texts + (size_t)n * rs, texts + (size_t)i * rs, (size_t)rs);
        }
        ++n;
    }
    *n_raw = n;
    if (n > max_raw) return fail(AIM_ENOMEM, "%u pairs must travel raw, side list holds %u", n, max_raw);
    return AIM_OK;
}

int aim_cigar_format_runs(const uint32_t *runs, uint32_t n_runs, char *out, int32_t cap)
{
    if (!runs || !out || cap < 4 || n_runs == 0) return fail(AIM_EINVAL, "bad arguments");
    return cigar_line(n_runs, [&](uint32_t i) { return (char)(runs[i] & 0xff); }, [&](uint32_t i) { return runs[i] >> 8; }, out, cap);
}

static inline uint64_t sm64(uint64_t *s)
{
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int aim_gen_pairs(uint64_t seed, uint64_t first_idx, uint32_t n_pairs, int32_t len, double error,
                  int32_t read_size, aim_request_t *requests, char *patterns, char *texts)
{
    if (!requests || !patterns || !texts || len <= 0 || read_size <= 0) return fail(AIM_EINVAL, "bad arguments");
    const int nedits = (int)std::ceil((double)len * error);
    if (len + nedits > read_size) return fail(AIM_EINVAL, "read_size %d too small for len %d + %d edits", read_size, len, nedits);
    static const char kBase[4] = {'A', 'C', 'G', 'T'};
    auto one = [&](uint32_t i) {
        uint64_t st = seed * 0xD1342543DE82EF95ull + (first_idx + i) * 0x2545F4914F6CDD1Dull + 0x632BE59BD9B4E019ull;
        char *p = patterns + (size_t)i * read_size;
        char *t = texts + (size_t)i * read_size;
        memset(p, 0, (size_t)read_size);
        memset(t, 0, (size_t)read_size);
        for (int j = 0; j < len; ++j) p[j] = kBase[sm64(&st) >> 62];
        memcpy(t, p, (size_t)len);
        int cur = len;
        for (int e = 0; e < nedits; ++e) {
            const uint64_t r = sm64(&st);
            const int kind = (int)((r >> 40) % 3);
            const char b = kBase[(r >> 32) & 3];
            if (kind == 0 && cur > 0) {          // substitute (may re-draw the same base)
                t[(r & 0xffffffffu) % (uint32_t)cur] = b;
            } else if (kind == 1 && cur > 0) {   // delete
                const int pos = (int)((r & 0xffffffffu) % (uint32_t)cur);
                memmove(t + pos, t + pos + 1, (size_t)(cur - pos - 1));
                t[--cur] = 0;
            } else {                             // insert
                const int pos = (int)((r & 0xffffffffu) % (uint32_t)(cur + 1));
                memmove(t + pos + 1, t + pos, (size_t)(cur - pos));
                t[pos] = b;
                ++cur;
            }
        }
        requests[i].pattern_len = len;
        requests[i].text_len = cur;
        requests[i].padding = 0;
        requests[i].idx = (uint32_t)(first_idx + i);
    };
    // pair i depends only on (seed, first_idx + i): long reads (each edit moves up to len bytes) are generated by all cores
    const uint64_t work = (uint64_t)n_pairs * (uint64_t)len * (uint64_t)(nedits + 1);
    unsigned nt = work > (1ull << 28) ? std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 64u) : 1u;
    if (nt > n_pairs) nt = n_pairs ? n_pairs : 1;
    if (nt <= 1) {
        for (uint32_t i = 0; i < n_pairs; ++i) one(i);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([&, t] { for (uint32_t i = t; i < n_pairs; i += nt) one(i); });
        for (auto &x : th) x.join();
    }
    return AIM_OK;
}

}  // extern "C"
