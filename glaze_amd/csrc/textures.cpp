// The texture pool and its lazy mip chain (textures.h).
#include "textures.h"

#include <algorithm>
#include <cstring>
#include <thread>

#include "mipchain.h"

namespace glz {

// 128-byte tiles: 8 x 4 RGBA texels or 16 x 8 gray texels (device/shading.h fetch_texel); ragged edges are padded
struct Tiling {
  uint32_t tw, th, bpp, tiles_x, tiles_y;
  Tiling(uint32_t format, uint32_t w, uint32_t h) {
    const bool gray = format == GLZ_TEX_GRAY;
    tw = gray ? 16u : 8u, th = gray ? 8u : 4u, bpp = gray ? 1u : 4u;
    tiles_x = (w + tw - 1) / tw, tiles_y = (h + th - 1) / th;
  }
  size_t bytes() const { return (size_t)tiles_x * tiles_y * 128u; }
};
// one image, tiled, appended to `pool` (whose size stays a multiple of 128)
static TexDesc append_tiled(std::vector<uint8_t>& pool, uint32_t format, uint32_t w, uint32_t h, const uint8_t* px) {
  const Tiling t(format, w, h);
  pool.resize((pool.size() + 127) & ~size_t(127));
  const size_t base = pool.size();
  pool.resize(base + t.bytes(), 0);
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      const size_t dst = base + ((size_t)(y / t.th) * t.tiles_x + x / t.tw) * 128u + ((size_t)(y % t.th) * t.tw + x % t.tw) * t.bpp;
      memcpy(&pool[dst], &px[((size_t)y * w + x) * t.bpp], t.bpp);
    }
  return TexDesc{(uint32_t)base, w, h, format | (t.tiles_x << 8)};
}

bool Textures::copy_of(const glz_texture* textures, uint32_t n, std::vector<TextureData>& out, Error& err) {
  if (n == 0 || !textures) return err.fail(GLZ_E_ARG, "the texture list must keep at least the default texture");
  std::vector<TextureData> fresh(n);
  for (uint32_t i = 0; i < n; ++i) {
    const glz_texture& t = textures[i];
    const size_t bytes = (size_t)t.width * t.height * (t.format == GLZ_TEX_GRAY ? 1 : 4);
    if (!t.pixels || !bytes || t.format < 1 || t.format > 3) return err.fail(GLZ_E_INVALID_DATA, "texture has inconsistent dimensions");
    fresh[i].info = t;
    fresh[i].level0.assign(t.pixels, t.pixels + bytes);
  }
  out.swap(fresh);
  for (auto& t : out) t.info.pixels = t.level0.data();
  return true;
}

bool Textures::upload(hipStream_t st, const std::vector<TextureData>& textures, Error& err) {
  std::vector<TexDesc> desc(textures.size());
  std::vector<uint8_t> pool;
  for (size_t i = 0; i < textures.size(); ++i) {
    const TextureData& t = textures[i];
    const size_t bytes = (size_t)t.info.width * t.info.height * (t.info.format == GLZ_TEX_GRAY ? 1 : 4);
    if (t.level0.size() < bytes || t.info.width == 0 || t.info.height == 0 || t.info.format < 1 || t.info.format > 3)
      return err.fail(GLZ_E_INVALID_DATA, "texture has inconsistent dimensions");
    const Tiling tiling(t.info.format, t.info.width, t.info.height);
    if (pool.size() + tiling.bytes() > 0xFFFFFFFFull || tiling.tiles_x >= (1u << 24)) return err.fail(GLZ_E_UNSUPPORTED, "texture pool larger than 4 GiB");
    // texel_address multiplies the tile row by tiles_x with a 24-bit multiply (2^24 tile rows are a strip of 2^26 texel rows or more)
    if (tiling.tiles_y >= (1u << 24)) return err.fail(GLZ_E_UNSUPPORTED, "texture of 2^24 tile rows or more");
    if (t.info.width == 1 && t.info.height == 1) {
      // the texel travels in the descriptor (device/shading.h kTexInline): materials' default maps cost no texel load
      uint32_t bits = 0;
      memcpy(&bits, t.level0.data(), tiling.bpp);
      desc[i] = TexDesc{bits, 1u, 1u, t.info.format | 0x80u | (1u << 8)};
      continue;
    }
    desc[i] = append_tiled(pool, t.info.format, t.info.width, t.info.height, t.level0.data());
  }
  // the texels change: whatever mip levels were built belong to the old ones
  mips_ready_ = false;
  h_mips_.clear();
  if (!hip_ok(d_desc_.upload(desc.data(), desc.size(), st), "upload texture descriptors", err)) return false;
  if (!hip_ok(d_pool_.upload(pool.data(), pool.size(), st), "upload texture pool", err)) return false;
  return hip_ok(hipStreamSynchronize(st), "texture upload", err);   // the staging vectors above must outlive the copies
}

bool Textures::ensure_mips(hipStream_t st, std::vector<TextureData>& textures, Error& err) {
  if (mips_ready_) return true;
  const size_t nt = textures.size();
  h_mips_.assign(nt, {});
  std::vector<std::vector<host::MipLevel>> chains(nt);
  std::vector<std::string> decode_errs(nt);
  auto build_one = [&](size_t i) {
    TextureData& t = textures[i];
    if (!t.decode_more_levels(decode_errs[i])) return;   // the file's own levels 1.., still PNG-encoded since parse
    std::vector<host::MipLevel> given(1);
    given[0].width = t.info.width;
    given[0].height = t.info.height;
    given[0].pixels = t.level0;
    for (size_t l = 0; l < t.more_levels.size(); ++l) {
      host::MipLevel m;
      m.width = t.more_dims[2 * l];
      m.height = t.more_dims[2 * l + 1];
      m.pixels = t.more_levels[l];
      given.push_back(std::move(m));
    }
    chains[i] = host::build_mip_chain(t.info.format, std::move(given));
  };
  const unsigned workers = (unsigned)std::min<size_t>(nt, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
  if (workers <= 1) {
    for (size_t i = 0; i < nt; ++i) build_one(i);
  } else {
    std::vector<std::thread> pool;
    std::vector<std::string> failed(workers);
    for (unsigned w = 0; w < workers; ++w)
      pool.emplace_back([&, w] {
        try {
          for (size_t i = w; i < nt; i += workers) build_one(i);
        } catch (const std::exception& ex) {
          failed[w] = ex.what();
        }
      });
    for (auto& th : pool) th.join();
    for (auto& f : failed)
      if (!f.empty()) return err.fail(GLZ_E_IO, "mip chain: " + f);
  }
  for (size_t i = 0; i < nt; ++i)
    if (!decode_errs[i].empty()) return err.fail(GLZ_E_INVALID_DATA, "Corrupted image: " + decode_errs[i]);
  std::vector<uint8_t> pool;
  std::vector<TexDesc> desc;
  std::vector<uint32_t> base(nt, 0);
  for (size_t i = 0; i < nt; ++i) {
    const uint32_t levels = (uint32_t)chains[i].size();
    base[i] = (uint32_t)desc.size() | (levels << 24);
    for (uint32_t l = 1; l < levels; ++l) {
      const host::MipLevel& m = chains[i][l];
      desc.push_back(append_tiled(pool, textures[i].info.format, m.width, m.height, m.pixels.data()));
      h_mips_[i].push_back(m.pixels);
    }
    if (pool.size() > 0xFFFFFFF0ull || desc.size() >= (1u << 24)) return err.fail(GLZ_E_UNSUPPORTED, "mip pool larger than 4 GiB");
  }
  if (!hip_ok(d_mip_desc_.upload(desc.data(), desc.size(), st), "upload mip descriptors", err)) return false;
  if (!hip_ok(d_mip_pool_.upload(pool.data(), pool.size(), st), "upload mip pool", err)) return false;
  if (!hip_ok(d_mip_base_.upload(base.data(), base.size(), st), "upload mip table", err)) return false;
  if (!hip_ok(hipStreamSynchronize(st), "mip upload", err)) return false;
  mips_ready_ = true;
  return true;
}

const std::vector<uint8_t>* Textures::mip_level(uint32_t texture, uint32_t level) const {
  if (!mips_ready_ || texture >= h_mips_.size() || level == 0 || level - 1 >= h_mips_[texture].size()) return nullptr;
  return &h_mips_[texture][level - 1];
}

void Textures::describe(DeviceScene& dev) const {
  dev.tex_desc = d_desc_.ptr;
  dev.tex_pool = d_pool_.ptr;
  dev.n_textures = (uint32_t)d_desc_.count;
  if (!mips_ready_) return;   // null until the chain is built, and again after an upload
  dev.tex_mip_desc = d_mip_desc_.ptr;
  dev.tex_mip_pool = d_mip_pool_.ptr;
  dev.tex_mip_base = d_mip_base_.ptr;
}

}  // namespace glz
