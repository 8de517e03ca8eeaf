// cosim_spawn.hip — placement kernel of the spawn table (cosim_spawn_set, include/cosim.h).
//
// A table row is a base pose (x, y, yaw) given by the user; the kernel finds the row's z so that the robot rests on the heightfield
// without penetrating it, and writes the pose (x, y, z, qw, qx, qy, qz, --) the reset block of env_body reads.
//
// Rule (its float64 numpy twin is cosim_amd/spawn.py place_reference).  The robot's footprint is one bounding sphere per ground geom
// at the nominal pose init_qpos: (ox, oy) horizontal offset of the centre from the base, r radius, `free` = how far the sphere's
// lowest point is above z = 0 there.  Yawed by the row, geom g's centre lies over g_xy = (x, y) + R(yaw) (ox, oy); hmax_g is the
// highest heightfield sample of the vertex window terrain_max_under defines for a sphere of radius r there.  The prism surface inside
// a cell never exceeds the cell's corner heights, so lifting the base by
//     dz = max(0, max_g(sz hmax_g - free_g)) + clearance
// leaves every point of every geom at least as far above the terrain as it was above z = 0 at the nominal pose.
//
// One wave64 per row.  The geoms are taken in turn; the lanes stride over the window's vertices row-major (a window row is contiguous
// in memory, so a wave's loads coalesce) and each keeps the largest sz h - free it has seen -- sz >= 0, so that is the window maximum
// applied to the rule -- then one cross-lane max and a store of the row by lane 0.  Windows are 2 x 2 vertices on the 55 cm cells of
// rocky_*, ~60 x 60 per geom on the 1 cm cells of the stairs; the maximum is exact at any size.  The host has checked every window to
// lie on the field (cosim_spawn_set), the clamps below keep a bad input from reading outside it all the same.  Cold: runs when the
// table is set, index arithmetic in double.
namespace cosim {

struct SpawnArgs {
  const float* xyyaw;     // [rows][3]
  const float4* foot;     // [n_foot]: ox, oy, r, free
  float* out;             // [rows][8]: x, y, z, qw, qx, qy, qz, 0
  const float* hfield;    // null on plane ground: dz = clearance
  int rows, n_foot, nrow, ncol;
  float sx, sy, sz, gx, gy;   // hfield_size[0..2], ground_pos[0..1]
  float init_z, clearance;
  float iq[4];            // init_qpos[3:7]
};

__global__ __launch_bounds__(64) void spawn_place_kernel(SpawnArgs a) {
  const int row = blockIdx.x, lane = threadIdx.x;
  if (row >= a.rows) return;
  const float x = a.xyyaw[3 * (size_t)row], y = a.xyyaw[3 * (size_t)row + 1], yaw = a.xyyaw[3 * (size_t)row + 2];
  const double c = cos((double)yaw), s = sin((double)yaw);
  float best = -3.0e38f;   // max over (geom, window vertex) of sz h - free, this lane's share
  if (a.hfield != nullptr) {
    const double dx = 2.0 * (double)a.sx / (double)(a.ncol - 1), dy = 2.0 * (double)a.sy / (double)(a.nrow - 1);
    for (int g = 0; g < a.n_foot; g++) {
      const float4 f = a.foot[g];
      const double rb = (double)f.z;
      const double lx = (double)x + (c * (double)f.x - s * (double)f.y) - (double)a.gx;
      const double ly = (double)y + (s * (double)f.x + c * (double)f.y) - (double)a.gy;
      int cmin = (int)floor((lx - rb + (double)a.sx) / dx), cmax = (int)ceil((lx + rb + (double)a.sx) / dx);
      int rmin = (int)floor((ly - rb + (double)a.sy) / dy), rmax = (int)ceil((ly + rb + (double)a.sy) / dy);
      cmin = min(max(cmin, 0), a.ncol - 1); cmax = min(max(cmax, 0), a.ncol - 1);
      rmin = min(max(rmin, 0), a.nrow - 1); rmax = min(max(rmax, 0), a.nrow - 1);
      const int w = cmax - cmin + 1;
      const int n = w * (rmax - rmin + 1);   // (at most nrow * ncol, which the host holds below 2^31)
      for (int i = lane; i < n; i += 64) {
        const int r = rmin + i / w, cc = cmin + i % w;
        best = fmaxf(best, a.sz * a.hfield[(size_t)r * (size_t)a.ncol + (size_t)cc] - f.w);
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = fmaxf(best, __shfl_xor(best, m, 64));
  if (lane == 0) {
    const float dz = fmaxf(0.f, best) + a.clearance;
    // q = q_yaw (x) init_quat in fp32; q_yaw = (cos(yaw / 2), 0, 0, sin(yaw / 2))
    const float hw = (float)cos(0.5 * (double)yaw), hz = (float)sin(0.5 * (double)yaw);
    float* o = a.out + 8 * (size_t)row;
    o[0] = x; o[1] = y; o[2] = a.init_z + dz;
    o[3] = hw * a.iq[0] - hz * a.iq[3];
    o[4] = hw * a.iq[1] - hz * a.iq[2];
    o[5] = hw * a.iq[2] + hz * a.iq[1];
    o[6] = hw * a.iq[3] + hz * a.iq[0];
    o[7] = 0.f;
  }
}

}  // namespace cosim
