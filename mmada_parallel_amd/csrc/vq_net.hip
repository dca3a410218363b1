// vq_net.hip — the image tokenizers of MMaDA-Parallel as networks of the kernels of vq_kernels.hip:
// the handle with its table of expected checkpoint tensors, the workspace plan and the two runs.  Host code only.
//   MAGVITv2.decode_code            models/modeling_magvitv2.py:429-433
//   LFQuantizer.get_codebook_entry  :208-221      VQGANDecoder.forward  :369-406
//   MAGVITv2.get_code               :422-427      VQGANEncoder.forward  :143-171
//   diffusers VQModel (A variant)   autoencoders/vq_model.py, autoencoders/vae.py (see include/mmada_mi355x.h)
// One Net record describes any of the four networks (taming / diffusers checkpoint, decoder / encoder); one builder
// registers its tensors under the key names of the checkpoint flavour, and the runs read nothing but the record.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/mmada_mi355x.h"
#include "vq.h"

namespace {

struct ConvP {
    float *w = nullptr, *b = nullptr;
    int co = 0, ci = 0, k = 0;
};
struct NormP {
    float *g = nullptr, *b = nullptr;
    int c = 0;
};
struct ResP {
    NormP n1, n2;
    ConvP c1, c2, nin;
    bool has_nin = false;
};
struct Slot {  // one expected state-dict tensor
    float** dst;
    long long numel;
    int co, ci, kk;  // conv weight: repack; otherwise kk = 0
    bool bound;
};

// What a network is; level 0 is the image resolution, level n_levels-1 the latent one (the taming numbering).
struct Net {
    bool encoder = false;       // image -> code (else code -> image)
    bool mid_attn = true;       // attention between the two mid res blocks
    bool learned_code = false;  // codebook [n_code, code_dim] (VQModel); else the lookup-free code of code_dim sign bits
    int n_levels = 0;
    int ch[8] = {}, blocks[8] = {};  // channels and res blocks per level
    int enc_stem = 0;           // channels out of the encoder's conv_in (taming: ch, whatever ch_mult[0] is)
    int image_ch = 0, latent_ch = 0, code_dim = 0, n_code = 0;
};

// The key fragments in which the taming (MAGVITv2) and the diffusers (VQModel) checkpoints differ; [0] decoder, [1] encoder
struct Names {
    const char* block[2];     // res block: level index, block index
    const char* resample[2];  // resample conv: level index
    bool up_reversed;         // the decoder's level index in a key runs against the level number (up_blocks.{L-1-lvl})
    const char* shortcut;
    const char* mid_res[2];
    const char *attn_norm, *attn_q, *attn_k, *attn_v, *attn_out;
    const char* norm_out;
    const char* quant[2];
};
const Names TAMING = {{"up.%d.block.%d", "down.%d.block.%d"}, {"up.%d.upsample.conv", "down.%d.downsample.conv"}, false,
                      "nin_shortcut", {"mid.block_1", "mid.block_2"},
                      "mid.attn_1.norm", "mid.attn_1.q", "mid.attn_1.k", "mid.attn_1.v", "mid.attn_1.proj_out",
                      "norm_out", {"post_quant_conv", "quant_conv"}};
// diffusers Attention with one head: GroupNorm, Linear q / k / v / out (= 1x1 convolutions), residual
const Names DIFFUSERS = {{"up_blocks.%d.resnets.%d", "down_blocks.%d.resnets.%d"},
                         {"up_blocks.%d.upsamplers.0.conv", "down_blocks.%d.downsamplers.0.conv"}, true,
                         "conv_shortcut", {"mid_block.resnets.0", "mid_block.resnets.1"},
                         "mid_block.attentions.0.group_norm", "mid_block.attentions.0.to_q", "mid_block.attentions.0.to_k",
                         "mid_block.attentions.0.to_v", "mid_block.attentions.0.to_out.0",
                         "conv_norm_out", {"post_quant_conv", "quant_conv"}};

}  // namespace

struct mmada_vq {
    Net net;
    ConvP quant, conv_in, conv_out, aq, ak, av, aproj;  // quant: post_quant_conv (decoder) / quant_conv (encoder)
    NormP norm_out, attn_norm;
    ResP mid1, mid2;
    std::vector<std::vector<ResP>> levels;  // [level][block]
    std::vector<ConvP> resample;            // [level] the conv that leaves the level: decoder level > 0, encoder level < L-1
    float* codebook = nullptr;              // [n_code, code_dim]
    std::map<std::string, Slot> slots;
    std::vector<float*> owned;
};

namespace {

void reg_conv(mmada_vq* h, const std::string& p, ConvP& c, int co, int ci, int k) {
    c.co = co; c.ci = ci; c.k = k;
    h->slots[p + ".weight"] = Slot{&c.w, (long long)co * ci * k * k, co, ci, k * k, false};
    h->slots[p + ".bias"] = Slot{&c.b, co, 0, 0, 0, false};
}
void reg_norm(mmada_vq* h, const std::string& p, NormP& n, int c) {
    n.c = c;
    h->slots[p + ".weight"] = Slot{&n.g, c, 0, 0, 0, false};
    h->slots[p + ".bias"] = Slot{&n.b, c, 0, 0, 0, false};
}
void reg_res(mmada_vq* h, const std::string& p, ResP& r, int ci, int co, const char* shortcut) {
    reg_norm(h, p + ".norm1", r.n1, ci);
    reg_conv(h, p + ".conv1", r.c1, co, ci, 3);
    reg_norm(h, p + ".norm2", r.n2, co);
    reg_conv(h, p + ".conv2", r.c2, co, co, 3);
    r.has_nin = ci != co;
    if (r.has_nin) reg_conv(h, p + "." + shortcut, r.nin, co, ci, 1);
}

std::string fmt_key(const char* pattern, int a, int b = 0) {
    char buf[96];
    snprintf(buf, sizeof buf, pattern, a, b);
    return buf;
}

// Registers every tensor of h->net under the names of `nm`, in the order the network runs.
//   decoder: quant conv, conv_in, mid, levels L-1 .. 0 (resample after all but the last), norm_out, conv_out
//            (VQGANDecoder.__init__ modeling_magvitv2.py:278-367; diffusers Decoder, autoencoders/vae.py)
//   encoder: conv_in, levels 0 .. L-1 (resample after all but the last), mid, norm_out, conv_out, quant conv
//            (VQGANEncoder.__init__ :62-141; diffusers Encoder, then VQModel.quant_conv)
void build_net(mmada_vq* h, const Names& nm) {
    const Net& n = h->net;
    const int L = n.n_levels, dir = n.encoder;
    h->levels.resize(L);
    h->resample.resize(L);
    if (n.learned_code)
        h->slots["quantize.embedding.weight"] = Slot{&h->codebook, (long long)n.n_code * n.code_dim, 0, 0, 0, false};
    int c = 0;  // channels of the running tensor
    auto level = [&](int lvl, bool last) {
        const int idx = (!n.encoder && nm.up_reversed) ? L - 1 - lvl : lvl;
        h->levels[lvl].resize(n.blocks[lvl]);
        for (int b = 0; b < n.blocks[lvl]; ++b) {
            reg_res(h, fmt_key(nm.block[dir], idx, b), h->levels[lvl][b], c, n.ch[lvl], nm.shortcut);
            c = n.ch[lvl];
        }
        if (!last) reg_conv(h, fmt_key(nm.resample[dir], idx), h->resample[lvl], c, c, 3);
    };
    auto mid = [&]() {
        reg_res(h, nm.mid_res[0], h->mid1, c, c, nm.shortcut);
        if (n.mid_attn) {
            reg_norm(h, nm.attn_norm, h->attn_norm, c);
            reg_conv(h, nm.attn_q, h->aq, c, c, 1);
            reg_conv(h, nm.attn_k, h->ak, c, c, 1);
            reg_conv(h, nm.attn_v, h->av, c, c, 1);
            reg_conv(h, nm.attn_out, h->aproj, c, c, 1);
        }
        reg_res(h, nm.mid_res[1], h->mid2, c, c, nm.shortcut);
    };
    if (!n.encoder) {
        reg_conv(h, nm.quant[0], h->quant, n.latent_ch, n.code_dim, 1);
        c = n.ch[L - 1];
        reg_conv(h, "conv_in", h->conv_in, c, n.latent_ch, 3);
        mid();
        for (int lvl = L - 1; lvl >= 0; --lvl) level(lvl, lvl == 0);
        reg_norm(h, nm.norm_out, h->norm_out, c);
        reg_conv(h, "conv_out", h->conv_out, n.image_ch, c, 3);
    } else {
        c = n.enc_stem;
        reg_conv(h, "conv_in", h->conv_in, c, n.image_ch, 3);
        for (int lvl = 0; lvl < L; ++lvl) level(lvl, lvl == L - 1);
        mid();
        reg_norm(h, nm.norm_out, h->norm_out, c);
        reg_conv(h, "conv_out", h->conv_out, n.latent_ch, c, 3);
        reg_conv(h, nm.quant[1], h->quant, n.code_dim, n.latent_ch, 1);
    }
}

// number of tensors never bound; *first: the key of the first one (in key order), if any
int unbound(const mmada_vq* h, const char** first = nullptr) {
    int n = 0;
    for (const auto& kv : h->slots)
        if (!kv.second.bound && n++ == 0 && first) *first = kv.first.c_str();
    return n;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Plan {
    size_t act_bytes;   // one activation buffer (largest [B, H, W, C] of the network)
    size_t attn_bytes;  // q, k, v, v^T ([T, C] each) + S [T, T], per batch element handled one at a time
    size_t gn_bytes;
    size_t total;
};

Plan plan_for(const Net& n, int B, int hz, int wz) {
    // largest [H, W, C] of the network: level l lives at hz * 2^(L-1-l); a tensor at that resolution has the channel
    // count of level l or of a neighbouring level (first block of a level / tensor just after a resample)
    size_t max_elems = 0;
    for (int lvl = 0; lvl < n.n_levels; ++lvl) {
        int c = n.ch[lvl];
        if (lvl > 0) c = std::max(c, n.ch[lvl - 1]);
        if (lvl + 1 < n.n_levels) c = std::max(c, n.ch[lvl + 1]);
        const size_t f = (size_t)1 << (n.n_levels - 1 - lvl);
        max_elems = std::max(max_elems, (size_t)hz * f * wz * f * c);
    }
    Plan p;
    p.act_bytes = align256(max_elems * B * sizeof(float));
    const size_t T = (size_t)hz * wz, C = (size_t)n.ch[n.n_levels - 1];
    p.attn_bytes = align256((4 * T * C * B + T * T) * sizeof(float));
    p.gn_bytes = align256(group_norm_scratch_bytes(B));
    p.total = 3 * p.act_bytes + p.attn_bytes + p.gn_bytes;
    return p;
}

// The workspace as a run uses it: three activation buffers, the attention scratch, the GroupNorm partials — in this order
struct Carve {
    float *x, *t1, *t2, *attn;
    double* gn;
};

// What decode and get_code check alike before the first launch, under the entry point's own name `who`: the attention
// rule on the latent grid (`grid`: how the entry point spells hz*wz), every tensor bound, the workspace large enough and
// aligned.  Then the carve.
int run_setup(const mmada_vq* h, const char* who, const char* grid, int B, int hz, int wz, void* workspace,
              size_t workspace_bytes, Carve& cv) {
    if (h->net.mid_attn && (hz * wz) % 32) return mm_fail("%s: %s must be a multiple of 32 (attention K tiles)", who, grid);
    const char* missing = nullptr;
    if (unbound(h, &missing)) return mm_fail("%s: tensor '%s' was never bound", who, missing);
    const Plan pl = plan_for(h->net, B, hz, wz);
    if (workspace_bytes < pl.total) return mm_fail("%s: workspace too small (%zu < %zu)", who, workspace_bytes, pl.total);
    if ((uintptr_t)workspace & 255) return mm_fail("%s: workspace must be 256-byte aligned", who);
    char* ws = (char*)workspace;
    cv.x = (float*)ws;
    cv.t1 = (float*)(ws + pl.act_bytes);
    cv.t2 = (float*)(ws + 2 * pl.act_bytes);
    cv.attn = (float*)(ws + 3 * pl.act_bytes);
    cv.gn = (double*)(ws + 3 * pl.act_bytes + pl.attn_bytes);
    return 0;
}

struct Runner {
    hipStream_t s;
    double* gn;
    int B;
    // resample: 0 same size, 1 = 2x nearest upsample folded in front, -1 = Downsample (pad right/bottom, stride 2)
    int conv(const ConvP& p, const float* in, float* out, const float* resid, int Hi, int Wi, int resample, int nchw = 0) {
        return launch_conv(conv_args(in, p.w, p.b, resid, out, B, Hi, Wi, p.ci, p.co, p.k, resample, nchw), s);
    }
    // out[i][j] = sum_k a[i][k] b[j][k] for a [M, K], b [N, K]: a 1x1 convolution of M pixels with b as its weights
    int matmul_nt(const float* a, const float* b, float* out, int M, int N, int K) {
        return launch_conv(conv_args(a, b, nullptr, nullptr, out, 1, M, 1, K, N, 1, 0), s);
    }
    // AttnBlock.forward (common_modules.py:187-211): x += proj_out(softmax(q k^T / sqrt(C)) v), single head over H*W
    int attn(const mmada_vq* h, float* x, float* t1, float* scratch, int H, int W) {
        const int T = H * W, C = h->attn_norm.c;
        float* q = scratch;
        float* k = q + (size_t)B * T * C;
        float* v = k + (size_t)B * T * C;
        float* vt = v + (size_t)B * T * C;   // one batch element at a time: [C, T]
        float* S = vt + (size_t)B * T * C;   // [T, T]
        if (norm(h->attn_norm, x, t1, T, 0)) return 1;
        if (conv(h->aq, t1, q, nullptr, H, W, 0)) return 1;
        if (conv(h->ak, t1, k, nullptr, H, W, 0)) return 1;
        if (conv(h->av, t1, v, nullptr, H, W, 0)) return 1;
        for (int b = 0; b < B; ++b) {
            const size_t off = (size_t)b * T * C;
            if (matmul_nt(q + off, k + off, S, T, T, C)) return 1;  // S[i][j] = sum_c q[i][c] k[j][c]
            if (launch_vq_softmax_rows(S, T, T, 1.0f / sqrtf((float)C), s)) return 1;
            if (launch_vq_transpose(v + off, vt, T, C, s)) return 1;
            if (matmul_nt(S, vt, t1 + off, T, C, T)) return 1;  // h_[i][c] = sum_j softmax(S)[i][j] v[j][c]
        }
        return conv(h->aproj, t1, x, x, H, W, 0);
    }
    int norm(const NormP& n, const float* in, float* out, int HW, int swish) {
        return launch_group_norm(in, n.g, n.b, out, gn, B, HW, n.c, swish, s);
    }
    // common_modules.py:337-357; x is updated in place (its channel count becomes r.c2.co)
    int res(const ResP& r, float* x, float* t1, float* t2, int H, int W) {
        if (norm(r.n1, x, t1, H * W, 1)) return 1;
        if (conv(r.c1, t1, t2, nullptr, H, W, 0)) return 1;
        if (norm(r.n2, t2, t1, H * W, 1)) return 1;
        if (r.has_nin) {
            if (conv(r.nin, x, t2, nullptr, H, W, 0)) return 1;
            return conv(r.c2, t1, x, t2, H, W, 0);
        }
        return conv(r.c2, t1, x, x, H, W, 0);
    }
    // the two mid res blocks with the attention between them (decoder :380-382, encoder :159-162)
    int mid(const mmada_vq* h, float* x, float* t1, float* t2, float* scratch, int H, int W) {
        if (res(h->mid1, x, t1, t2, H, W)) return 1;
        if (h->net.mid_attn && attn(h, x, t1, scratch, H, W)) return 1;
        return res(h->mid2, x, t1, t2, H, W);
    }
};

int check_cfg(const mmada_vq_cfg* cfg, mmada_vq** out) {
    if (!cfg || !out) return mm_fail("mmada_vq_create: null argument");
    if (cfg->n_levels < 1 || cfg->n_levels > 8) return mm_fail("mmada_vq_create: n_levels must be 1..8");
    if (cfg->ch <= 0 || cfg->ch % 128) return mm_fail("mmada_vq_create: ch must be a positive multiple of 128 (GroupNorm(32) over float4 columns)");
    if (cfg->z_channels <= 0 || cfg->z_channels > 62 || cfg->out_ch <= 0 || cfg->out_ch > 16)
        return mm_fail("mmada_vq_create: bad z_channels / out_ch");
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->ch_mult[i] <= 0 || cfg->num_res_blocks[i] <= 0 || cfg->ch * cfg->ch_mult[i] > 1024)
            return mm_fail("mmada_vq_create: bad ch_mult / num_res_blocks at level %d", i);
    return 0;
}

// MAGVITv2 (taming keys, lookup-free code of z_channels bits); an encoder's cfg->out_ch carries its image channels
int create_magvit(const mmada_vq_cfg* cfg, bool encoder, mmada_vq** out) {
    if (check_cfg(cfg, out)) return 1;
    mmada_vq* h = new mmada_vq();
    Net& n = h->net;
    n.encoder = encoder;
    n.n_levels = cfg->n_levels;
    for (int i = 0; i < cfg->n_levels; ++i) {
        n.ch[i] = cfg->ch * cfg->ch_mult[i];
        n.blocks[i] = cfg->num_res_blocks[i];
    }
    n.enc_stem = cfg->ch;
    n.image_ch = cfg->out_ch;
    n.latent_ch = n.code_dim = cfg->z_channels;
    build_net(h, TAMING);
    *out = h;
    return 0;
}

}  // namespace

extern "C" {

int mmada_vq_create(const mmada_vq_cfg* cfg, mmada_vq** out) { return create_magvit(cfg, false, out); }

/* VQGANEncoder.__init__ (modeling_magvitv2.py:62-141); cfg->out_ch carries in_ch (image channels) */
int mmada_vq_create_encoder(const mmada_vq_cfg* cfg, mmada_vq** out) { return create_magvit(cfg, true, out); }

/* ---- diffusers VQModel (A variant): learned codebook, optional mid-block attention ------------------------------------ */
int mmada_vq_create_vqmodel(const mmada_vqmodel_cfg* cfg, int encoder, mmada_vq** out) {
    if (!cfg || !out) return mm_fail("mmada_vq_create_vqmodel: null argument");
    const int L = cfg->n_levels;
    if (L < 1 || L > 8) return mm_fail("mmada_vq_create_vqmodel: 1..8 blocks, got %d", L);
    if (cfg->norm_num_groups != GN_GROUPS) return mm_fail("mmada_vq_create_vqmodel: norm_num_groups must be %d", GN_GROUPS);
    if (cfg->layers_per_block < 1 || cfg->layers_per_block > 16) return mm_fail("mmada_vq_create_vqmodel: bad layers_per_block");
    if (cfg->latent_channels <= 0 || cfg->latent_channels > 1024 || cfg->vq_embed_dim <= 0 || cfg->vq_embed_dim > 1024 ||
        cfg->num_vq_embeddings <= 0 || cfg->image_channels <= 0 || cfg->image_channels > 16)
        return mm_fail("mmada_vq_create_vqmodel: bad latent_channels / vq_embed_dim / num_vq_embeddings / image_channels");
    for (int i = 0; i < L; ++i)
        if (cfg->block_out_channels[i] <= 0 || cfg->block_out_channels[i] % 128 || cfg->block_out_channels[i] > 1024)
            return mm_fail("mmada_vq_create_vqmodel: block_out_channels[%d]=%d must be a multiple of 128 up to 1024 "
                           "(GroupNorm(32) over float4 columns)", i, cfg->block_out_channels[i]);
    mmada_vq* h = new mmada_vq();
    Net& n = h->net;
    n.encoder = encoder != 0;
    n.mid_attn = cfg->mid_block_add_attention != 0;
    n.learned_code = true;
    n.n_levels = L;
    for (int i = 0; i < L; ++i) {  // level l of the taming numbering = diffusers block l; a Decoder block has one more layer
        n.ch[i] = cfg->block_out_channels[i];
        n.blocks[i] = cfg->layers_per_block + (encoder ? 0 : 1);
    }
    n.enc_stem = n.ch[0];
    n.image_ch = cfg->image_channels;
    n.latent_ch = cfg->latent_channels;
    n.code_dim = cfg->vq_embed_dim;
    n.n_code = cfg->num_vq_embeddings;
    build_net(h, DIFFUSERS);
    *out = h;
    return 0;
}

void mmada_vq_destroy(mmada_vq* h) {
    if (!h) return;
    for (float* p : h->owned) (void)hipFree(p);
    delete h;
}

int mmada_vq_bind(mmada_vq* h, const char* name, const float* data, int64_t numel, void* stream) {
    if (!h || !name || !data) return mm_fail("mmada_vq_bind: null argument");
    std::string key(name);
    const std::string prefix = h->net.encoder ? "encoder." : "decoder.";
    if (key.rfind(prefix, 0) == 0) key = key.substr(prefix.size());
    auto it = h->slots.find(key);
    if (it == h->slots.end()) return mm_fail("mmada_vq_bind: unexpected tensor '%s'", name);
    Slot& sl = it->second;
    if (numel != sl.numel) return mm_fail("mmada_vq_bind: '%s' has %lld elements, expected %lld", name, (long long)numel, sl.numel);
    hipStream_t s = (hipStream_t)stream;
    if (!*sl.dst) {
        float* p = nullptr;
        MM_CHECK_HIP(hipMalloc(&p, (size_t)numel * sizeof(float)));
        h->owned.push_back(p);
        *sl.dst = p;
    }
    if (sl.kk > 1) {
        if (launch_vq_repack_conv(data, *sl.dst, sl.co, sl.ci, sl.kk, s)) return 1;
    } else {
        MM_CHECK_HIP(hipMemcpyAsync(*sl.dst, data, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    sl.bound = true;
    return 0;
}

int mmada_vq_num_unbound(const mmada_vq* h) { return h ? unbound(h) : -1; }

size_t mmada_vq_workspace_bytes(const mmada_vq* h, int B, int hz, int wz) {
    if (!h || B <= 0 || hz <= 0 || wz <= 0) return 0;
    return plan_for(h->net, B, hz, wz).total;  // encoder: the same buffers (largest activation is at the image resolution)
}

int mmada_vq_decode_code(mmada_vq* h, const int64_t* indices, int B, int hz, int wz, void* workspace,
                         size_t workspace_bytes, float* out, void* stream) {
    if (!h || !indices || !workspace || !out) return mm_fail("mmada_vq_decode_code: null argument");
    const Net& n = h->net;
    if (n.encoder) return mm_fail("mmada_vq_decode_code: this handle is an encoder");
    if (B <= 0 || hz <= 0 || wz <= 0) return mm_fail("mmada_vq_decode_code: bad shape");
    Carve cv;
    if (run_setup(h, "mmada_vq_decode_code", "hz*wz", B, hz, wz, workspace, workspace_bytes, cv)) return 1;
    hipStream_t s = (hipStream_t)stream;
    Runner r{s, cv.gn, B};
    float *x = cv.x, *t1 = cv.t1, *t2 = cv.t2;
    int H = hz, W = wz;
    const long long npix = (long long)B * H * W;

    // get_codebook_entry (:208-221) -> post_quant_conv -> conv_in (:374-377)
    if (n.learned_code) {  // VectorQuantizer.get_codebook_entry: rows of the learned codebook, already NHWC
        if (launch_vq_gather(indices, h->codebook, t1, npix, n.code_dim, n.n_code, s)) return 1;
    } else {
        if (launch_vq_lfq_entry(indices, t1, npix, n.code_dim, s)) return 1;
    }
    if (r.conv(h->quant, t1, t2, nullptr, H, W, 0)) return 1;
    if (r.conv(h->conv_in, t2, x, nullptr, H, W, 0)) return 1;
    if (r.mid(h, x, t1, t2, cv.attn, H, W)) return 1;
    // upsampling (:385-391)
    for (int lvl = n.n_levels - 1; lvl >= 0; --lvl) {
        for (const ResP& rb : h->levels[lvl])
            if (r.res(rb, x, t1, t2, H, W)) return 1;
        if (lvl != 0) {
            if (r.conv(h->resample[lvl], x, t1, nullptr, H, W, 1)) return 1;
            std::swap(x, t1);
            H *= 2; W *= 2;
        }
    }
    // end (:398-400); output NCHW like the reference
    if (r.norm(h->norm_out, x, t1, H * W, 1)) return 1;
    return r.conv(h->conv_out, t1, out, nullptr, H, W, 0, 1);
}

/* MAGVITv2.get_code (modeling_magvitv2.py:422-427): VQGANEncoder.forward (:143-171) -> sign quantisation -> indices */
int mmada_vq_get_code(mmada_vq* h, const float* pixel_values, int B, int H, int W, void* workspace,
                      size_t workspace_bytes, int64_t* indices_out, float* z_out, void* stream) {
    if (!h || !pixel_values || !workspace || !indices_out) return mm_fail("mmada_vq_get_code: null argument");
    const Net& n = h->net;
    if (!n.encoder) return mm_fail("mmada_vq_get_code: this handle is a decoder");
    const int f = 1 << (n.n_levels - 1);
    if (B <= 0 || H <= 0 || W <= 0 || H % f || W % f) return mm_fail("mmada_vq_get_code: H, W must be multiples of %d", f);
    char grid[48];
    snprintf(grid, sizeof grid, "(H/%d)*(W/%d)", f, f);
    Carve cv;
    if (run_setup(h, "mmada_vq_get_code", grid, B, H / f, W / f, workspace, workspace_bytes, cv)) return 1;
    hipStream_t s = (hipStream_t)stream;
    Runner r{s, cv.gn, B};
    float *x = cv.x, *t1 = cv.t1, *t2 = cv.t2;
    if (launch_vq_nchw_to_nhwc(pixel_values, t1, B, n.image_ch, (long long)H * W, s)) return 1;
    if (r.conv(h->conv_in, t1, x, nullptr, H, W, 0)) return 1;
    int Hc = H, Wc = W;
    for (int lvl = 0; lvl < n.n_levels; ++lvl) {  // downsampling (:148-156); hs[-1] is always the running tensor
        for (const ResP& rb : h->levels[lvl])
            if (r.res(rb, x, t1, t2, Hc, Wc)) return 1;
        if (lvl != n.n_levels - 1) {
            if (r.conv(h->resample[lvl], x, t1, nullptr, Hc, Wc, -1)) return 1;
            std::swap(x, t1);
            Hc /= 2; Wc /= 2;
        }
    }
    if (r.mid(h, x, t1, t2, cv.attn, Hc, Wc)) return 1;
    if (r.norm(h->norm_out, x, t1, Hc * Wc, 1)) return 1;  // end (:165-169)
    if (r.conv(h->conv_out, t1, t2, nullptr, Hc, Wc, 0)) return 1;
    if (r.conv(h->quant, t2, t1, nullptr, Hc, Wc, 0)) return 1;  // quant_conv
    const long long npix = (long long)B * Hc * Wc;
    if (n.learned_code) {  // VQModel.encode -> latents [npix, code_dim]; VectorQuantizer: nearest codebook row
        if (launch_vq_nearest_code(t1, h->codebook, indices_out, npix, n.code_dim, n.n_code, s)) return 1;
    } else {
        if (launch_vq_lfq_index(t1, indices_out, npix, n.code_dim, s)) return 1;
    }
    if (z_out) MM_CHECK_HIP(hipMemcpyAsync(z_out, t1, (size_t)npix * n.code_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

int mmada_vq_nearest_code(mmada_vq* h, const float* z_nhwc, int64_t n, int64_t* indices_out, void* stream) {
    if (!h || !z_nhwc || !indices_out) return mm_fail("mmada_vq_nearest_code: null argument");
    if (!h->net.learned_code || !h->codebook) return mm_fail("mmada_vq_nearest_code: needs a VQModel handle with its codebook bound");
    if (n <= 0) return 0;
    return launch_vq_nearest_code(z_nhwc, h->codebook, indices_out, n, h->net.code_dim, h->net.n_code, (hipStream_t)stream);
}

}  // extern "C"
