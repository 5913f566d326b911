// The tile partition rule, on the host: who owns which 64 x 64 tile of a frame.  The one definition behind the renderer's launches
// (renderer.cpp) and the device-free entry points glz_host_tile_owner / glz_host_chain_owner (abi.cpp).  Host code only: the kernels
// read the TileMap they are handed (kernels.h).
#pragma once
#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace glz {

constexpr uint32_t kTile = 64;   // a tile's edge in pixels

// Partition (rank, world) of a w x h frame: tiles are numbered row by row, rank owns the global tiles t with t % world == rank
// (its local tile j = global tile rank + j * world), every local tile takes kTile * kTile pixel slots whether the frame clips it or not.
inline TileMap make_tile_map(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
  TileMap m{};
  m.width = w;
  m.height = h;
  m.tiles_x = (w + kTile - 1) / kTile;
  m.tiles_y = (h + kTile - 1) / kTile;
  m.rank = rank;
  m.world = world;
  const uint32_t tiles = m.tiles_x * m.tiles_y;
  m.n_local_tiles = world != 0 && tiles > rank ? (tiles - rank + world - 1) / world : 0;
  m.n_local_pixels = m.n_local_tiles * kTile * kTile;
  return m;
}
// chain s of S concurrent chains of partition (rank, world) renders the finer partition (rank + s * world, world * S)
inline TileMap make_chain_map(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t s, uint32_t S) {
  return make_tile_map(w, h, rank + s * world, world * S);
}

inline uint32_t tile_of_pixel(const TileMap& m, uint32_t x, uint32_t y) { return (y / kTile) * m.tiles_x + x / kTile; }
inline uint32_t tile_owner(uint32_t t, uint32_t world) { return t % world; }
// which of its owner's S chains renders tile t: the s with t % (world * S) == rank + s * world
inline uint32_t tile_chain(uint32_t t, uint32_t world, uint32_t S) { return (t % (world * S)) / world; }

// pixels of the frame (not slots) inside the tiles the map's rank owns
inline uint64_t owned_pixels(const TileMap& m) {
  uint64_t owned = 0;
  for (uint32_t t = m.rank; t < m.tiles_x * m.tiles_y; t += m.world) {
    const uint32_t tx = t % m.tiles_x, ty = t / m.tiles_x;
    owned += (uint64_t)std::min(kTile, m.width - tx * kTile) * std::min(kTile, m.height - ty * kTile);
  }
  return owned;
}

}  // namespace glz
