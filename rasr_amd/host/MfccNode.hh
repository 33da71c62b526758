// rasr_amd/host/MfccNode.hh -- header-only C++ mirror of the mfcc.flow sub-network as ONE node on top of the C
// ABI.  It follows the Flow::Node life cycle (src/Flow/Node.hh:37-185): setParameter(name, value) with the
// parameter names of the replaced nodes, configure() (reads "sample-rate", publishes the output attributes of
// signal-cosine-transform / signal-window: sample-rate = 1, frame-shift, datatype = vector-f32), then per segment
// putSamples()* / eos() / getFeature()* -- the pull loop of Speech::FeatureExtractor::processSegment
// (src/Speech/DataExtractor.cc:101-111) sees one Flow::Vector<f32> per frame with the reference's timestamps.
#ifndef RASR_AMD_HOST_MFCC_NODE_HH
#define RASR_AMD_HOST_MFCC_NODE_HH

#include <cstdlib>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/amx.h"

namespace AmxHost {

struct FeaturePacket {  // Flow::Vector<f32> + Flow::Timestamp
    std::vector<float> data;
    double             startTime, endTime;
};

class MfccNode {
    amx_ctx*                           ctx_;
    amx_mfcc_cfg                       cfg_;
    amx_mfcc*                          h_;
    amx_mfcc_info                      info_;
    std::vector<float>                 samples_;
    std::vector<int16_t>               samples16_;
    double                             segmentStart_;
    std::vector<float>                 ceps_;
    long                               nFrames_, next_;
    std::map<std::string, std::string> outputAttributes_;
    // VTLN: warping-function = nest(linear-2(<factor> | $(warping-factor), <limit>), mel | bark); the filter bank of the factor in
    // force is rebuilt when a segment brings another one (Flow::StringExpressionNode)
    bool        vtln_ = false, factorFromParameter_ = false;
    double      vtlnLimit_ = 0, warpingFactor_ = 1, builtFactor_ = 0;
    std::string error_;

public:
    /** The warping-function declarations this node accepts: "mel", "bark" and
     *  "nest(linear-2(<factor>|$(warping-factor), <limit>), mel|bark)" (blanks ignored).  Anything else of
     *  Math/AnalyticFunctionFactory's grammar (other nestings, mel(discretize-argument), linear-3, bilinear, ...) is refused:
     *  false and a message in *error.  factor = 0 when it comes from $(warping-factor). */
    static bool parseWarpingFunction(const std::string& declaration, int* warping, bool* vtln, double* factor, double* limit,
                                     std::string* error) {
        std::string d;
        for (char c : declaration)
            if (c != ' ' && c != '\t')
                d += c;
        *vtln   = false;
        *factor = 1;
        *limit  = 0;
        auto outer = [&](const std::string& w) {
            if (w == "mel")
                *warping = AMX_WARP_MEL;
            else if (w == "bark")
                *warping = AMX_WARP_BARK;
            else
                return false;
            return true;
        };
        if (outer(d))
            return true;
        const std::string head = "nest(linear-2(", param = "$(warping-factor)";
        size_t            pos  = 0;
        if (d.compare(0, head.size(), head) == 0) {
            pos = head.size();
            char* end = nullptr;
            if (d.compare(pos, param.size(), param) == 0) {
                *factor = 0;
                pos += param.size();
            }
            else {
                *factor = strtod(d.c_str() + pos, &end);
                if (end == d.c_str() + pos || !(*factor > 0)) {
                    *error = "warping-function \"" + declaration + "\": the warping factor must be a number > 0 or $(warping-factor)";
                    return false;
                }
                pos = (size_t)(end - d.c_str());
            }
            if (pos < d.size() && d[pos] == ',') {
                *limit = strtod(d.c_str() + pos + 1, &end);
                if (end != d.c_str() + pos + 1 && *limit > 0 && *limit < 1) {
                    pos = (size_t)(end - d.c_str());
                    if (d.compare(pos, 2, "),") == 0 && d.size() > pos + 3 && d.back() == ')' && outer(d.substr(pos + 2, d.size() - pos - 3))) {
                        *vtln = true;
                        return true;
                    }
                }
                else {
                    *error = "warping-function \"" + declaration + "\": the limit of linear-2 has to lie in the interval (0, 1)";
                    return false;
                }
            }
        }
        *error = "warping-function \"" + declaration + "\" is not supported: mel, bark or nest(linear-2(<factor>|$(warping-factor), <limit>), mel|bark)";
        return false;
    }
    /** the message of the last refused setParameter / configure of this node */
    const std::string& error() const { return error_; }

    static std::string filterName() { return "signal-mfcc-amx"; }

    explicit MfccNode(amx_ctx* ctx)
            : ctx_(ctx), h_(nullptr), segmentStart_(0), nFrames_(0), next_(0) {
        amx_mfcc_default_cfg(&cfg_);
    }
    ~MfccNode() { amx_mfcc_destroy(h_); }

    /** parameter names of the replaced nodes: alpha (signal-preemphasis), shift / length (signal-window),
     *  maximum-input-size / apply-scale (signal-real-fast-fourier-transform), filter-width / spacing /
     *  warp-differential-unit (signal-filterbank), nr-outputs / normalize (signal-cosine-transform) */
    bool setParameter(const std::string& name, const std::string& value) {
        const double v = atof(value.c_str());
        const bool   b = value == "true" || value == "yes" || value == "1";
        if (name == "alpha") cfg_.preemph_alpha = v;
        else if (name == "shift") cfg_.win_shift_s = v;
        else if (name == "length") cfg_.win_len_s = v;
        else if (name == "maximum-input-size") cfg_.fft_max_input_s = v;
        else if (name == "apply-scale") cfg_.apply_scale = b;
        else if (name == "filter-width") cfg_.mel_filter_width = v;
        else if (name == "spacing") cfg_.mel_spacing = v;
        else if (name == "warp-differential-unit") cfg_.warp_differential_unit = b;
        else if (name == "nr-outputs") cfg_.n_ceps = atoi(value.c_str());
        else if (name == "normalize") cfg_.dct_normalize = b;
        else if (name == "warping-function") {
            int    w = cfg_.warping;
            bool   vt;
            double f, l;
            if (!parseWarpingFunction(value, &w, &vt, &f, &l, &error_))
                return false;
            cfg_.warping = w, vtln_ = vt, vtlnLimit_ = l;
            factorFromParameter_ = vt && f == 0;
            if (vt && f != 0)
                warpingFactor_ = f;
        }
        else if (name == "warping-factor") {  // per segment, e.g. from a corpus key map; takes effect at the next segment's eos()
            if (!(v > 0)) {
                error_ = "warping-factor \"" + value + "\" is not a number > 0";
                return false;
            }
            if (!factorFromParameter_) {
                error_ = "warping-factor is set, but warping-function does not name $(warping-factor)";
                return false;
            }
            warpingFactor_ = v;
        }
        else return false;
        return true;
    }

    /** inputAttributes must carry "sample-rate" (samples.flow).  false + amx_last_error() on a bad configuration
     *  (the reference nodes call criticalError with the same texts). */
    bool configure(const std::map<std::string, std::string>& inputAttributes) {
        auto it = inputAttributes.find("sample-rate");
        cfg_.sample_rate = it == inputAttributes.end() ? 0.0 : atof(it->second.c_str());
        amx_mfcc_destroy(h_);
        h_ = nullptr;
        if (!createHandle())
            return false;
        outputAttributes_                = inputAttributes;
        outputAttributes_["sample-rate"] = "1";
        outputAttributes_["datatype"]    = "vector-f32";
        char buf[64];
        snprintf(buf, sizeof buf, "%g", cfg_.win_shift_s);
        outputAttributes_["frame-shift"] = buf;
        return true;
    }
    const std::map<std::string, std::string>& outputAttributes() const { return outputAttributes_; }

    /** one input packet of the `samples` stream; the first packet of a segment fixes its start time */
    void putSamples(const float* x, size_t n, double startTime) {
        if (samples_.empty() && next_ == nFrames_)
            segmentStart_ = startTime;
        samples_.insert(samples_.end(), x, x + n);
    }

    /** the same for a `vector-s16` stream, i.e. with the node linked straight behind the audio reader instead of behind
     *  generic-convert-vector-s16-to-vector-f32 (Flow/TypeConverter.hh:35-43 widens without scaling; the kernel does the same):
     *  half the bytes to the device.  A segment is all-s16 or all-f32. */
    void putSamples(const int16_t* x, size_t n, double startTime) {
        if (samples16_.empty() && next_ == nFrames_)
            segmentStart_ = startTime;
        samples16_.insert(samples16_.end(), x, x + n);
    }

    /** end of the segment's input: runs the fused kernel over the whole segment */
    bool eos() {
        if (!h_)
            return false;
        if (vtln_ && warpingFactor_ != builtFactor_) {  // a new warping factor: the filter bank of this one
            amx_mfcc_destroy(h_);
            h_ = nullptr;
            if (!createHandle()) {
                samples_.clear();
                samples16_.clear();
                nFrames_ = next_ = 0;
                nSamples_ = 0;
                return false;
            }
        }
        if (!samples_.empty() && !samples16_.empty()) {  // a segment is all-s16 or all-f32: drop it, the node stays usable for the next one
            samples_.clear();
            samples16_.clear();
            nFrames_ = next_ = 0;
            nSamples_ = 0;
            return false;
        }
        const bool s16 = !samples16_.empty();
        nSamples_      = (long)(s16 ? samples16_.size() : samples_.size());
        nFrames_       = amx_mfcc_n_frames(h_, nSamples_);
        next_          = 0;
        ceps_.assign((size_t)nFrames_ * info_.n_ceps, 0.f);
        const int r = s16 ? amx_mfcc_run_s16(h_, samples16_.data(), nSamples_, ceps_.data()) : amx_mfcc_run(h_, samples_.data(), nSamples_, ceps_.data());
        samples_.clear();
        samples16_.clear();
        return r == AMX_OK;
    }

    /** next feature packet; false = end of segment (Flow::Data::eos()) */
    bool getFeature(FeaturePacket& out) {
        if (next_ >= nFrames_)
            return false;
        out.data.assign(ceps_.begin() + next_ * info_.n_ceps, ceps_.begin() + (next_ + 1) * info_.n_ceps);
        const long remaining = nSamples_ - next_ * info_.frame_shift;
        const long len       = remaining < info_.frame_len ? remaining : info_.frame_len;
        out.startTime        = segmentStart_ + amx_mfcc_frame_start_time(h_, next_);
        out.endTime          = out.startTime + (double)len / cfg_.sample_rate;  // WindowBuffer::copy
        ++next_;
        return true;
    }

private:
    long nSamples_ = 0;

    bool createHandle() {
        int r;
        if (vtln_) {
            const amx_mfcc_vtln v = {vtlnLimit_, 1, &warpingFactor_};
            r            = amx_mfcc_create_vtln(ctx_, &cfg_, &v, &h_);
            builtFactor_ = warpingFactor_;
        }
        else
            r = amx_mfcc_create(ctx_, &cfg_, &h_);
        if (r != AMX_OK) {
            error_ = amx_last_error();
            h_     = nullptr;
            return false;
        }
        amx_mfcc_describe(h_, &info_);
        return true;
    }
};

}  // namespace AmxHost
#endif
