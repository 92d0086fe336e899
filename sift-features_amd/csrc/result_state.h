// The result-state rule of a context (include/sift_mi.h "Call sequence"): what
// the last producing call left behind, and which later calls may read it.  Where
// a result lives is a fact recorded by the call that produced it; the
// keep_on_device SETTING only chooses the destination of the next
// sift_mi_extract_batch_device.  Plain C++ with no HIP in it, so that the same
// text is api.cpp's, pipeline.cpp's and a stand-alone program's for the
// sanitizers (tests/host_result_state_main.cpp; tests/call_model.py restates the
// table).
//
//   call                                needs           on success
//   extract, extract_batch              -               where = host, pyramid = false,
//                                                       batch_readback = one chunk
//   extract_batch_device                -               where = keep ? device : host, else as above
//   precompute                          -               pyramid = true, where = none, batch_readback = false
//   sift_with_precomputed               pyramid         where = host, batch_readback = false, pyramid stays
//   fetch, fetch_keys                   where == host   unchanged
//   device_results                      where == device unchanged
//   octave_dims, read_scale_space/_dog  pyramid         unchanged
//   batch_octave_dims, read_batch_...   batch_readback  unchanged
//   set_keep_on_device                  -               keep only
//   set_max_octaves                     -               pyramid = false, batch_readback = false
//
// An unmet need is SIFT_MI_ESTATE and changes nothing; a call refused for its
// arguments before any buffer is touched changes nothing; a producing call that
// fails later (the plan replaced, an arena or a stage buffer rewritten) leaves
// where = none, pyramid = false, batch_readback = false.
#pragma once
#include <cstddef>

namespace siftmi {

enum class ResultWhere : int { none = 0, host = 1, device = 2 };
enum class ProducingCall : int { extract = 0, extract_device = 1, precompute = 2, with_precomputed = 3 };

// Wrong != 0 breaks one transition on purpose, for the test that shows the
// enumerated call sequences see every rule (tests/test_host_result_state.py);
// the library uses ResultState = ResultStateT<0> only.  1-3 are the behaviour
// this header replaced.
//   1 fetch consults keep              4 precompute keeps where
//   2 device_results consults keep     5 a late failure keeps pyramid
//   3 set_keep moves where             6 set_max_octaves keeps batch_readback
template <int Wrong = 0>
struct ResultStateT {
    ResultWhere where = ResultWhere::none;
    size_t n = 0;                 // rows of the result (0 while where == none)
    bool pyramid = false;         // the precomputed planes of one frame are in arena 0
    bool batch_readback = false;  // the last extraction ran as one chunk: its planes can be read back
    bool keep = false;            // sift_mi_set_keep_on_device

    // ---- needs ------------------------------------------------------------
    bool can_fetch() const {
        if (Wrong == 1) return where != ResultWhere::none && !keep;
        return where == ResultWhere::host;
    }
    bool can_device_results() const {
        if (Wrong == 2) return where != ResultWhere::none && keep;
        return where == ResultWhere::device;
    }
    bool can_read_pyramid() const { return pyramid; }
    bool can_read_batch() const { return batch_readback; }
    bool can_begin(ProducingCall c) const { return c != ProducingCall::with_precomputed || pyramid; }

    // ---- settings ---------------------------------------------------------
    void set_keep(bool k) {
        keep = k;
        if (Wrong == 3 && where != ResultWhere::none) where = k ? ResultWhere::device : ResultWhere::host;
    }
    void set_max_octaves() {
        pyramid = false;  // the plan is rebuilt on the next call
        if (Wrong != 6) batch_readback = false;
    }

    // ---- producing calls --------------------------------------------------
    // Where the call about to run puts its rows: device memory only for
    // device-resident frames under the keep setting.
    ResultWhere destination(ProducingCall c) const {
        return c == ProducingCall::extract_device && keep ? ResultWhere::device : ResultWhere::host;
    }
    // The call succeeded with `rows` rows at `dest` (= destination(c) when it began).
    void done(ProducingCall c, ResultWhere dest, size_t rows, bool one_chunk) {
        if (c == ProducingCall::precompute) {
            if (Wrong != 4) {
                where = ResultWhere::none;
                n = 0;
            }
            pyramid = true;
            batch_readback = false;
            return;
        }
        where = dest;
        n = rows;
        if (c == ProducingCall::with_precomputed) {
            batch_readback = false;  // (pyramid stays: the planes were only read)
        } else {
            pyramid = false;
            batch_readback = one_chunk;
        }
    }
    // The call failed after it had touched a buffer: nothing is readable.
    void failed_late() {
        where = ResultWhere::none;
        n = 0;
        if (Wrong != 5) pyramid = false;
        batch_readback = false;
    }
};

using ResultState = ResultStateT<0>;

// A producing call from its first touched buffer on: unless done() is reached,
// every way out is a late failure.
template <int Wrong = 0>
struct ProducingScope {
    ResultStateT<Wrong>& s;
    bool finished = false;
    explicit ProducingScope(ResultStateT<Wrong>& state) : s(state) {}
    ProducingScope(const ProducingScope&) = delete;
    ProducingScope& operator=(const ProducingScope&) = delete;
    void done(ProducingCall c, ResultWhere dest, size_t rows, bool one_chunk) {
        s.done(c, dest, rows, one_chunk);
        finished = true;
    }
    ~ProducingScope() {
        if (!finished) s.failed_late();
    }
};

}  // namespace siftmi
