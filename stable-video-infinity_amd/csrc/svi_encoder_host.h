// svi_encoder_host.h — what the three once-per-clip encoders (svi_encoders.hip: umT5, CLIP; svi_wav2vec.hip: wav2vec2) share on the host: the weight
// table an encoder describes ONCE as data, the workspace arena, and each forward's buffer list.  No device code and no HIP call in here.
#pragma once

#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "svi_common.h"

// ---- weight table -------------------------------------------------------------------------------------------------------------------
// A row is a state-dict key (or, with ENC_LAYER, the part after "<layer_prefix><i>.") and its shape for this handle's configuration.
enum : unsigned {
    ENC_LAYER = 1,       // one per layer 0 .. layers - 1; layers >= layers_used are accepted and unused (CLIP's last block)
    ENC_UNUSED = 2,      // accepted (any shape) and never read
    ENC_ABSENT = 4,      // not a key of this configuration (T5: which pos_embedding exists follows shared_pos)
};
struct EncRow { std::string name; std::vector<int64_t> shape; unsigned flags; };

struct EncTable {
    const char* noun = "";                      // "text encoder": every message names it
    const char* bind_fn = "";                   // the entry point that binds, for its bad-argument message
    svi_dtype dtype = SVI_F32;                  // the one dtype parameters come in, and how the refusal words it
    const char* dtype_words = "";
    int max_rank = 0;
    std::string layer_prefix;
    int layers = 0, layers_used = 0;
    std::vector<EncRow> rows;                   // plain rows and per-layer rows, each group in check_bound's order
    std::map<std::string, const void*> bound;

    // the row `name` spells, or null; *used = false where the name is accepted and ignored
    const EncRow* find(const std::string& name, bool* used) const {
        for (const EncRow& r : rows)
            if (!(r.flags & (ENC_LAYER | ENC_ABSENT)) && r.name == name) { *used = !(r.flags & ENC_UNUSED); return &r; }
        if (name.rfind(layer_prefix, 0) != 0) return nullptr;
        const char* s = name.c_str() + layer_prefix.size();
        char* end = nullptr;
        const long i = strtol(s, &end, 10);
        if (end == s || *end != '.' || i < 0 || i >= layers) return nullptr;
        for (const EncRow& r : rows)
            if ((r.flags & (ENC_LAYER | ENC_ABSENT)) == ENC_LAYER && r.name == end + 1) { *used = i < layers_used && !(r.flags & ENC_UNUSED); return &r; }
        return nullptr;
    }
    // every name a forward reads: the plain rows, then layer by layer
    std::vector<std::string> keys() const {
        std::vector<std::string> k;
        for (const EncRow& r : rows) if (!r.flags) k.push_back(r.name);
        for (int i = 0; i < layers_used; ++i)
            for (const EncRow& r : rows) if (r.flags == ENC_LAYER) k.push_back(layer_prefix + std::to_string(i) + "." + r.name);
        return k;
    }
    svi_status bind(const char* name, const void* dev_ptr, svi_dtype dt, const int64_t* shape, int32_t rank) {
        SVI_REQUIRE(name && dev_ptr && shape && rank >= 1 && rank <= max_rank, "%s: bad argument", bind_fn);
        SVI_REQUIRE(dt == dtype, "%s parameter '%s' must be %s", noun, name, dtype_words);
        SVI_REQUIRE(((uintptr_t)dev_ptr % 16) == 0, "%s parameter '%s' is not 16-byte aligned", noun, name);
        bool used = true;
        const EncRow* r = find(name, &used);
        if (!r) { svi_set_error("unknown %s parameter '%s'", noun, name); return SVI_ERR_INVALID; }
        if (!used) return SVI_OK;
        bool ok = (size_t)rank == r->shape.size();
        for (int i = 0; ok && i < rank; ++i) ok = shape[i] == r->shape[i];
        if (!ok) { svi_set_error("shape mismatch for %s parameter '%s'", noun, name); return SVI_ERR_INVALID; }
        bound[name] = dev_ptr;
        return SVI_OK;
    }
    svi_status unbound(const std::string& name) const { svi_set_error("%s parameter '%s' was never bound", noun, name.c_str()); return SVI_ERR_UNBOUND; }
    svi_status check_bound() const {
        for (const auto& k : keys())
            if (!bound.count(k)) return unbound(k);
        return SVI_OK;
    }
    // looks up, never inserts: a name the forward misspells is SVI_ERR_UNBOUND, not a null pointer handed to a kernel
    template <typename T> svi_status get(const std::string& name, const T** out) const {
        const auto it = bound.find(name);
        if (it == bound.end()) return unbound(name);
        *out = static_cast<const T*>(it->second);
        return SVI_OK;
    }
};
// the bound pointer of `name` as const T*; on a miss the CALLING function returns SVI_ERR_UNBOUND before the expression it stands in is evaluated further
#define SVI_ENC_W(T, table, name) ({ const T* enc_w_; SVI_TRY((table).get<T>(name, &enc_w_)); enc_w_; })

// ---- handle base, workspace -----------------------------------------------------------------------------------------------------------
struct EncHandle {
    int device = -1;                            // SVI_REQUIRE_DEVICE
    EncTable w;
    char* ws = nullptr; size_t ws_bytes = 0;
};
// at least `need` bytes of workspace (svi_encoder_kernels.hip); hipFree waits for the work that still reads the old one
svi_status svi_enc_grow(EncHandle* h, size_t need);

// Slices of one allocation, each 256-byte aligned.  Without a base it only measures: take() returns null and `used` is the size to allocate.
struct EncArena {
    char* base; size_t used = 0;
    explicit EncArena(char* b = nullptr) : base(b) {}
    template <typename T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};
// `buffers(arena)` states a forward's buffers once: run to measure, then again on the grown workspace to hand out the pointers
template <typename F> svi_status svi_enc_carve(EncHandle* h, F&& buffers) {
    EncArena measure;
    buffers(measure);
    SVI_TRY(svi_enc_grow(h, measure.used));
    EncArena carve(h->ws);
    buffers(carve);
    return SVI_OK;
}

// ---- the three buffer lists (order = layout) -------------------------------------------------------------------------------------------
struct T5Bufs { bf16 *X, *N, *Q, *K, *V, *A, *G, *F1; };                     // R rows: residual, normed, q, k, v, attention, gate, fc1
inline T5Bufs t5_buffers(EncArena& a, size_t R, size_t dim, size_t da, size_t df) {          // (a braced list is evaluated left to right)
    return {a.take<bf16>(R * dim), a.take<bf16>(R * dim), a.take<bf16>(R * da), a.take<bf16>(R * da), a.take<bf16>(R * da), a.take<bf16>(R * da),
            a.take<bf16>(R * df), a.take<bf16>(R * df)};
}
struct ClipBufs { float *P, *X0, *N, *A, *QKV, *H; };                        // np patches of kp values; T = np + 1 token rows
inline ClipBufs clip_buffers(EncArena& a, size_t np, size_t kp, size_t T, size_t dim, size_t md) {
    return {a.take<float>(np * kp), a.take<float>(T * dim), a.take<float>(T * dim), a.take<float>(T * dim), a.take<float>(T * 3 * dim), a.take<float>(T * md)};
}
// n samples, t1 / t2 frames after the first / second convolution layer (A and B hold the layers' outputs alternately), S output frames.  Part: the partial
// sums, one per `chunk` rows, of the waveform's statistics (one column) or the GroupNorm's (C columns).  Big is q | k | v and then the feed-forward's hidden rows.
struct W2vBufs { float *Wv, *A, *B, *Part, *Stat, *I0, *I1, *X, *Y, *N1, *At, *Big; };
inline W2vBufs w2v_buffers(EncArena& a, size_t n, size_t t1, size_t t2, size_t chunk, size_t S, size_t C, size_t H, size_t F) {
    return {a.take<float>(n), a.take<float>(t1 * C), a.take<float>(t2 * C),
            a.take<float>(std::max((n + chunk - 1) / chunk, (t1 + chunk - 1) / chunk * C)), a.take<float>(2 * std::max<size_t>(C, 1)),
            a.take<float>(S * C), a.take<float>(S * C), a.take<float>(S * H), a.take<float>(S * H), a.take<float>(S * H), a.take<float>(S * H),
            a.take<float>(S * std::max(F, 3 * H))};
}
