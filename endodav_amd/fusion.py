"""Surface fusion on the GPU (opt-in): a depth video with its poses integrated into one truncated signed distance (TSDF) volume, and the zero
crossings of that volume as one coloured point list, as one coloured, oriented, indexed triangle mesh, or as depth, normal and colour maps seen from given cameras; and the camera tracked against that volume where the video comes without poses.  Not in the reference, whose ``3d_reconstruction`` clouds concatenate every frame's points:
a thousand re-observations of the same tissue, each frame's depth noise a shell of its own.  Here every voxel averages what the frames saw.

``Volume`` says where the voxels are; ``Tsdf`` owns the arrays on the GPU (``edv_tsdf_integrate`` / ``edv_tsdf_count`` / ``edv_tsdf_extract``,
include/endodav_hip.h) and ``TsdfHost`` is its numpy mirror, the same operations in the same order, so the two agree bit for bit.  The clip,
its depth rule, mask and cameras are a ``cloud.Cloud`` with ``step = 1``:

  state     ``tsdf``, ``weight`` float32 [nz, ny, nx] and optionally ``color`` float32 [nz, ny, nx, 3]; fresh: tsdf = 1, weight = 0, color = 0
  cameras   formed once on the host in float64 and handed to both implementations: W = rows 0..2 of ``np.linalg.inv`` of the 4x4 pose
            T_world_camera, and rows 0 and 1 of K (whose last row must be [0, 0, 1])
  integrate one thread per voxel, the frames in order.  Per voxel (i_x, i_y, i_z) and frame, every operation rounded separately:
            float64  c_a = origin_a + (i_a + 0.5) * voxel;  q_i = ((W[i,0]*c_x + W[i,1]*c_y) + W[i,2]*c_z) + W[i,3];  skip unless q_2 > 0
            float64  u = ((K00*q_0 + K01*q_1) + K02*q_2) / q_2, v likewise from row 1 (pixel centres at (x + 0.5, y + 0.5), the cloud's
                     convention);  skip unless 0 <= u < w and 0 <= v < h;  px = int(u), py = int(v)
            float32  z and the keep predicate of pixel (py, px) are the cloud's (module docstring of ``cloud``);  skip if not kept
            float64  sdf = float64(z) - q_2;  skip if sdf < -trunc;  d = float32(min(1, sdf / trunc))
            float32  wn = weight + 1;  tsdf = (tsdf*weight + d) / wn;  color = (color*weight + float32(rgb)) / wn;  weight = min(wn, max_weight)
  surface   voxel a in linear order (x fastest), axis k in x, y, z, b the neighbour of a along +k inside the grid; the pair emits a point when
            both weights are >= min_weight and (tsdf_a < 0) != (tsdf_b < 0), with 0 and -0 non-negative:
            float32  t = tsdf_a / (tsdf_a - tsdf_b)
            float64  p_k = origin_k + ((i_k + 0.5) + float64(t)) * voxel, the other two coordinates the voxel centre's, stored as float32
            float32  c = c_a + t * (c_b - c_a);  colour = uint8(min(255, max(0, floor(c + 0.5))))
            ordered voxel-major, axis-minor

  mesh      marching tetrahedra on the Kuhn split of every cell (``Tsdf.mesh`` / ``TsdfHost.mesh`` -> ``Mesh``; ``edv_tsdf_mesh_count`` /
            ``edv_tsdf_mesh_extract``).  Six tetrahedra around the body diagonal, the same in every cell, so neighbouring cells agree on the
            diagonals of their shared faces: a 16-case rule with no ambiguous case and a watertight, consistently oriented mesh, at up to 12
            triangles a cell.
            corners   corner c in 0..7 of a cell has offset off(c) = (c&1, c>>1&1, c>>2&1) in (x, y, z), which is also its linear hop.  Voxel a is
                      observed when weight[a] >= min_weight and inside when tsdf[a] < 0 (0 and -0 are outside, as for the surface).
            cells     the cell of voxel a exists when i_x+1 < nx, i_y+1 < ny and i_z+1 < nz; it is valid when its eight corners are observed.
                      Only valid cells emit triangles.
            vertices  voxel a owns the seven edges a -> a + off(d), d = 1..7: three axis edges, three face diagonals, the body diagonal.  Edge
                      (a, d) carries a vertex when b = a + off(d) is in the grid, a and b are observed, inside(a) != inside(b), and a valid
                      cell contains the edge: the cell of a - off(s) for some s in 0..7 with s & d == 0 that lies in the grid.  Ordered
                      voxel-major (x fastest), d-minor; every vertex is referenced by a triangle.
            float32   t = tsdf_a / (tsdf_a - tsdf_b)
            float64   p_k = origin_k + (d_k ? (i_k + 0.5) + float64(t) : (i_k + 0.5)) * voxel, stored as float32
            float32   colour exactly the surface's: c = c_a + t * (c_b - c_a);  uint8(min(255, max(0, floor(c + 0.5))))
            float32   normal, every operation rounded separately: the gradient of a voxel is g_k = tsdf[i_k -> min(i_k+1, n_k-1)] -
                      tsdf[i_k -> max(i_k-1, 0)] (no division; unobserved voxels contribute their stored value, a fresh one 1);
                      n_k = g_k(a) + t * (g_k(b) - g_k(a));  s = (n_x*n_x + n_y*n_y) + n_z*n_z;  len = sqrt(s), correctly rounded;
                      n_k / len if len > 0, otherwise (0, 0, 0).  Normals point to the positive side, free space: the side the triangles face.
            tetrahedra  for the permutations (p, q, r) of (0, 1, 2) in lexicographic order the corners (c0, c1, c2, c3) = (0, 1<<p,
                      (1<<p)|(1<<q), 7); bit i of the case mask m is set when corner c_i is inside.
            triangles  ins and outs the corner positions i, ascending.  m = 0 or 15: nothing.  One inside a: the polygon [(a, o) for o in outs];
                      one outside o: [(i, o) for i in ins]; two inside a < b and two outside c < d: [(a, c), (a, d), (b, d), (b, c)].  With
                      the polygon's points at the edge midpoints of the unit cube, the list is reversed if (P1-P0) x (P2-P0) . (mean of the
                      outside corners - mean of the inside corners) < 0.  Emitted: (P0, P1, P2) and for a quad also (P0, P2, P3).  Polygon
                      edge (i, j) is the cube edge between corners c_i and c_j: the smaller corner u is the owner's offset, d = v - u, and the
                      triangle stores the index of that vertex.  Ordered cell-major (linear index of the cell's voxel), then tetrahedron,
                      then the one or two triangles; int32.  ``MESH_TABLE`` holds the 6 x 16 rule, derived from this text at import.
            Degenerate cases stay: tsdf_a == 0 gives t = 0, so several vertices coincide and some triangles have zero area; the topology is
            unaffected and nothing is filtered.

  views     the volume as cameras see it (``Views``, ``Tsdf.raycast`` / ``TsdfHost.raycast`` -> ``Raycast``; ``edv_tsdf_raycast``): one thread per
            pixel marches its ray in equal steps of the cloud's depth and stops where the interpolated distance turns negative between two
            neighbouring valid samples.  Every operation is rounded on its own; no division in the march.
            setup     the cameras are ``Cloud(K=..., pose=...).cams(m)``: 21 doubles a view, Kinv, R and t, formed once on the host and handed
                      to both implementations; inv = 1.0 / voxel in float64, formed once on the host;
                      steps = floor((far - near) / step) + 1 in float64 in Python, at most ``MAX_STEPS``; step = the voxel unless given
            float64   per pixel (x, y) of view f:  u = x + 0.5, v = y + 0.5;  l_i = (Kinv[i,0]*u + Kinv[i,1]*v) + Kinv[i,2];
                      r_i = (R[i,0]*l_0 + R[i,1]*l_1) + R[i,2]*l_2 (the cloud's ray: a point at depth z is t + r*z);
                      o_i = (t_i - origin_i) * inv - 0.5 and d_i = r_i * inv: the ray in voxel-centre coordinates
            sample    at parameter z, float64:  g_i = o_i + d_i * z;  inside when 0 <= g_i <= n_i - 1 for i = x, y, z (NaN fails);
                      c_i = min(max(int(g_i), 0), n_i - 2);  f_i = float32(g_i - float64(c_i));  valid when inside and the eight voxels
                      c + off(0..7) all have weight >= min_weight
            float32   along x: a00 = v000 + f_x*(v100 - v000), and a10, a01, a11 likewise for (y+1), (z+1), (y+1, z+1);
                      along y: b0 = a00 + f_y*(a10 - a00), b1 = a01 + f_y*(a11 - a01);  along z: s = b0 + f_z*(b1 - b0)
            march     k = 0 .. steps-1 with z_k = near + float64(k) * step (not accumulated).  Sample k not valid: the previous sample is
                      forgotten.  Valid and not s < 0 (0 and -0 are outside, as everywhere here): (s, k) is remembered as the previous
                      sample.  Valid, s < 0 and sample k-1 remembered: a hit.  Valid and s < 0 otherwise: the ray ends as a miss (it entered
                      the surface from unobserved space, or started inside).  The steps run out: a miss.
            hit       float32 t = s_prev / (s_prev - s), the divisor positive;  float64 z* = z_{k-1} + float64(t) * step;
                      depth = float32(z*).  (c, f) again from z* by the formulas above (the clamp keeps them defined whatever the rounding);
                      weights are not consulted again, as the mesh's gradient takes stored values.
            float32   normal: the gradients g_k of the eight corners (the mesh's, no division), each component interpolated in the order
                      above;  (n_x*n_x + n_y*n_y) + n_z*n_z, sqrt, n_k / len if len > 0, otherwise (0, 0, 0): exactly the mesh's.
                      colour: the eight stored colours interpolated per channel in the same order;  uint8(min(255, max(0, floor(c + 0.5))))
            miss      depth 0, normal (0, 0, 0), colour (0, 0, 0).  Every pixel of every output is written exactly once, hit or miss.  A
                      volume with some n_i = 1 has no cell: every pixel is a miss.
            The depth is the cloud's: ``cloud.lift(depth, Cloud(K, pose, source="depth"))`` puts the hits back in the world.

  tracking  the pose of a frame found against the volume (``Track``, ``Tsdf.track`` / ``TsdfHost.track``, ``track_clip`` -> ``Tracked``;
            ``edv_icp_sums``, ``edv_icp_scaled_sums``): frame-to-model point-to-plane ICP with projective association.  The volume is ray-cast once from the guess (one
            view with normals: the model); then ``iterations`` times the normal equations are summed on the GPU (``icp_sums``; ``icp_sums_host``
            is the mirror), solved on the host (``icp_solve``) and the twist applied (``apply_twist``).  Solve and twist are plain float64 numpy
            and the same functions for both classes, so a whole track differs only in where the sums came from.
            pixel     output pixel (oy, ox) of the cloud's grid of the live frame; z (float32) and kept are the cloud's.  float64, every
                      operation rounded on its own, with Kinv, R, t of the current estimate:
                      u = (ox + 0.5) * step, v = (oy + 0.5) * step;  l_i = (Kinv[i,0]*u + Kinv[i,1]*v) + Kinv[i,2];
                      r_i = (R[i,0]*l_0 + R[i,1]*l_1) + R[i,2]*l_2;  rho_i = r_i * float64(z);  P_i = t_i + rho_i
            project   into the model's view exactly as integrate projects a voxel centre (W, K of ``cameras``):
                      q_i = ((W[i,0]*P_x + W[i,1]*P_y) + W[i,2]*P_z) + W[i,3];  skip unless q_2 > 0;
                      um = ((K00*q_0 + K01*q_1) + K02*q_2) / q_2, vm likewise;  skip unless 0 <= um < mw and 0 <= vm < mh;  px = int(um), py = int(vm)
            model     dm = depth[py, px], skip unless dm > 0 (a miss is 0);  N = float64(normals[py, px]), skip unless (N_x*N_x + N_y*N_y) + N_z*N_z > 0;
                      the vertex is the cloud's lift of the model's own pixel centre (px + 0.5, py + 0.5) at depth dm through the model's
                      Kinv, R, t:  V_i = t_m,i + rm_i * float64(dm);  D_i = V_i - P_i;  skip unless (D_x*D_x + D_y*D_y) + D_z*D_z <= max_dist^2
            terms     e = (N_x*D_x + N_y*D_y) + N_z*D_z;  c = rho x N (each product rounded, then the difference);  J = (c, N): the twist is
                      about the live camera centre, which keeps the system well conditioned far from the world origin.  29 terms a pixel:
                      J_j*J_k for j <= k, row-major (21), J_j*e (6), e*e, 1.  A pixel without a pair contributes 29 times +0.
            sums      float64, no atomics, a fixed order: tiles of 256 output pixels in row-major order, a wave 64 of them; inside a wave a
                      butterfly (s = 32, 16, 8, 4, 2, 1: x <- x + x[lane ^ s]), the tile ((w0 + w1) + w2) + w3, then the tiles in index order
                      starting from tile 0's value.  sums[28] is the number of pairs, sqrt(sums[27] / sums[28]) their rms distance to the planes.
            solve     the symmetric 6 x 6 system by ``np.linalg.solve``; lost when there are fewer than ``min_pairs`` pairs, the solve raises or
                      the solution is not finite.  A lost frame returns its guess.
            twist     xi = (rotation vector, translation):  R <- Rodrigues(xi[:3]) @ R, t <- t + xi[3:].  After the last step R is replaced by
                      U @ Vt of its SVD.
            clip      ``track_clip``: the Cloud holds one pose, the first camera's.  Frame 0 is integrated there; each later frame is tracked from
                      the previous frame's pose and integrated at the pose found; a lost frame keeps the previous pose and is not integrated.
            A scene that is a plane leaves sliding inside the plane unobservable; that is not detected ("colour" below sees it).
            scale     ``Track(scale=True)`` (``edv_icp_scaled_sums``): monocular depth is fixed only up to a scale that wanders from frame to
                      frame, and a tracker that takes every frame in the volume's unit trades that scale for rotation and translation.  With the
                      option the frame's scale is a seventh unknown.  Off (the default), everything above is unchanged to the bit.
                      where     the scale is the Cloud's ``gain``, the one place the depth rule has for it.  For a scale factor sigma (a Python
                                float) the frame is read with gain32 = float32(spec.gain * sigma), the product formed in Python doubles and rounded
                                once, as ``Cloud.scalars()`` does: z (float32) and kept are the cloud's for that gain, near and far applied to the
                                scaled depth.  The sums take no new scalar, and ``integrate`` sees exactly the z the tracker saw.
                      pixel     up to e and J_0..J_5 the rule above, character for character.  The seventh column, float64, every operation
                                rounded on its own:  J_6 = (rho_x*N_x + rho_y*N_y) + rho_z*N_z.  Growing the scale by delta moves P by delta*rho,
                                so e falls by delta*J_6: the sign convention of the translation columns.
                      terms     37 a pixel: [0..27] J_j*J_k for 0 <= j <= k <= 6, the upper triangle row-major; [28..34] J_j*e, j = 0..6; [35] e*e;
                                [36] 1.  A pixel without a pair contributes 37 times +0.
                      sums      exactly as above: tiles of 256, a butterfly per wave, ((w0 + w1) + w2) + w3, the tiles in index order from tile
                                0's value.  The 29 values the 6-column sums also have come out with the same bits for the same inputs.
                      solve     the symmetric 7 x 7 system by ``np.linalg.solve``, x = (rotation vector, translation, delta); lost as above.
                      update    T <- apply_twist(T, x[:6]), then sigma <- sigma * (1.0 + x[6]).  The frame is also lost when sigma is not finite
                                and positive, or when sigma / sigma_guess leaves [1/(1+m), 1+m] with m = ``Track.max_scale_step``.  A lost frame
                                returns its guess, pose and scale factor 1.0.  After the last step R is re-orthonormalised as above.
                      clip      frame 0 fixes the gauge, sigma_0 = 1.  Frame i is tracked from the previous frame's pose and scale: its Cloud
                                carries gain = spec.gain * sigma_{i-1} and the factor starts at 1;  sigma_i = sigma_{i-1} * factor;  it is
                                integrated with gain = spec.gain * sigma_i at the pose found.  A lost frame keeps the previous pose and scale and
                                is not integrated.  ``Tracked.scales`` holds sigma_i.
            colour    ``Track(colour=lambda)`` (``edv_icp_colour_sums``; ``icp_colour_sums`` / ``icp_colour_sums_host``): the sliding that
                      geometry cannot see is seen by colour.  The volume is coloured, so the model view has a colour image, and the live
                      frame has its RGB: every geometric pair also compares the two intensities, and a second block of sums holds the normal
                      equations of that residual.  Off (``None``, the default), everything above is unchanged to the bit.  Needs a coloured
                      volume and the clip's ``frames``; works with and without ``scale``.
                      pixel     through the distance test, e and J the rule above, character for character; a pixel without a geometric pair has
                                no colour pair either.  Then, float64, every operation rounded on its own:
                                gu = um - 0.5, gv = vm - 0.5;  skip unless mw >= 2, mh >= 2, 0 <= gu <= mw-1 and 0 <= gv <= mh-1;
                                x0 = min(int(gu), mw-2), y0 = min(int(gv), mh-2);  fx = gu - x0, fy = gv - y0;
                                skip unless the four model pixels (y0+j, x0+i) all have depth > 0 (a miss's colour is no colour)
                      intensity Y = (0.299*R + 0.587*G) + 0.114*B of a uint8 triple; I00, I10, I01, I11 of the model's four colours (Iij at
                                (y0+j, x0+i)), Yl of the live frame at the source pixel the depth was read from
                      sample    top = I00 + fx*(I10-I00);  bot = I01 + fx*(I11-I01);  Im = top + fy*(bot-top);
                                Iu = (I10-I00) + fy*((I11-I01) - (I10-I00));  Iv = (I01-I00) + fx*((I11-I10) - (I01-I00)): the patch's exact gradient
                      gradient  a = K00*q_0 + K01*q_1, b = K10*q_0 + K11*q_1;  gq_0 = (Iu*K00 + Iv*K10) / q_2;  gq_1 = (Iu*K01 + Iv*K11) / q_2;
                                gq_2 = -((Iu*a + Iv*b) / (q_2*q_2));  in the world g_j = (W[0,j]*gq_0 + W[1,j]*gq_1) + W[2,j]*gq_2
                      terms     r = Yl - Im; moving P by delta raises the model's intensity by g . delta, so r falls by g . delta, the sign
                                convention of e and N.  Jc = (rho x g, g), and with ``scale`` Jc_6 = (rho_x*g_x + rho_y*g_y) + rho_z*g_z.  The
                                geometric block's layout with Jc for J and r for e; +0 throughout where there is no colour pair.
                      sums      2 T values, T = 29 or 37: [0..T) the geometric block, with the bits ``icp_sums`` gives, [T..2T) the colour block;
                                the same tiles, butterfly, wave order and tile order.  sums[2T-1] is the number of colour pairs.
                      solve     A = A_g + lambda^2 * A_c, b = b_g + lambda^2 * b_c, formed on the host in float64, then ``icp_solve`` as above.
                                lambda weighs one intensity unit (of 255) against one unit of length.  ``pairs``, ``rms``, ``min_pairs`` and the
                                lost rules stay the geometric block's; no colour pairs adds nothing.
            robust    ``Track(min_cos=..., huber=..., huber_colour=...)`` (``edv_frame_normals``, ``edv_icp_robust_sums``; ``frame_normals`` /
                      ``frame_normals_host``, ``icp_robust_sums`` / ``icp_robust_sums_host``): the steps above believe every pair that passes the
                      distance test, and a highlight, an instrument or tissue that moved gives pairs that pass it.  A pair is tested against the
                      model twice more: by orientation, the live frame's own normal against the model's, and by the size of its residual, a Huber
                      weight.  All three off (``None``, the default), everything above is unchanged to the bit and the kernels above run; works
                      with and without ``scale`` and ``colour``.  float64, every operation rounded on its own.
                      normals   the live frame's normal map on the cloud's output grid, in the camera's frame, so it does not depend on the pose:
                                vertex   V_i = l_i * float64(z) with u, v, l as in "pixel" above, z (float32) and kept the cloud's
                                valid    1 <= ox <= ow-2, 1 <= oy <= oh-2, and the pixel and its neighbours (oy, ox-1), (oy, ox+1), (oy-1, ox), (oy+1, ox) kept
                                normal   a = V(oy, ox+1) - V(oy, ox-1);  b = V(oy+1, ox) - V(oy-1, ox);  c = b x a, each product rounded, then the
                                         difference: with x right, y down and z forward it points towards the camera, the free side, as the
                                         model's normals do;  s = (c_0*c_0 + c_1*c_1) + c_2*c_2;  len = sqrt(s);  n_i = float32(c_i / len) if len > 0
                                A pixel that is not valid or has len = 0 gets (0, 0, 0).  One thread a pixel and frame; the tracker forms the map of
                                its own frame once, before the first iteration, with the gain of the guess.  With ``scale`` it is not formed again
                                when the gain changes: a uniform scale does not turn a normal, only the kept set at the near and far edge can differ.
                      test      after the distance test, when ``min_cos`` is given:  nl = float64(map[oy, ox]);  skip unless (nl_0*nl_0 + nl_1*nl_1) + nl_2*nl_2 > 0;
                                nw_i = (R[i,0]*nl_0 + R[i,1]*nl_1) + R[i,2]*nl_2 with R of the current estimate;  skip unless
                                (N_0*nw_0 + N_1*nw_1) + N_2*nw_2 >= min_cos.  A skipped pixel has no pair and no colour pair.
                      weight    w = 1.0 if |e| <= huber, otherwise huber / |e|;  Jw_j = w * J_j;  the terms are Jw_j*J_k, Jw_j*e, then e*e
                                unweighted and 1: ``pairs`` and ``rms`` keep their meaning, the layout stays 29 / 37 and ``icp_solve`` is unchanged.
                                Since 1.0 * x == x, a pair inside the threshold contributes the bits of the plain kernel.  The colour block
                                likewise with r, ``huber_colour`` and Jc; r*r stays unweighted.  A threshold that is not given is +inf: w = 1.
                      sums      exactly as above: the same tiles, butterfly, wave order and tile order; no atomics.
                      Measured on the mirror (tests/test_track_robust_cpu.py): a block of 12.5 % of the live frame 0.04 nearer ends 2.37e-2 rad /
                      1.40e-2 from the truth with the plain tracker and 5.5e-3 / 3.8e-3 with huber = 0.005; the block replaced by a tilted plane
                      8.5e-3 / 3.1e-3 against 1.3e-3 / 6.8e-4 with min_cos = 0.985.
            pyramid   ``Track(pyramid=(i_0, ..., i_L), jump=...)`` (``edv_depth_pyramid``, ``edv_rgb_pyramid``; ``depth_pyramid`` / ``depth_pyramid_host``,
                      ``rgb_pyramid`` / ``rgb_pyramid_host``): coarse to fine.  Every step above runs on the live frame's full grid against a model
                      cast at full size.  A step at half size works on a quarter of the pixels and rays, and with large pixels the same motion is
                      a small displacement, which is what projective association needs.  ``pyramid`` lists the steps per level, finest first;
                      ``None`` (the default): everything above is unchanged to the bit and the same kernels run.
                      levels    level 0 is the cloud's grid of the live frame; it needs ``step == 1``, float32(near) >= 0 and gain > 0.  Level l+1
                                has size (h_l // 2, w_l // 2): an odd last row or column is dropped.  Every level must hold a pixel; at most
                                ``PYRAMID_MAX_LEVELS`` levels in all (the library's constant: the kernel's tile of level 0 is 2^(that - 1) pixels a
                                side).  K_l = diag(2^-l, 2^-l, 1) K, exactly: a power of two, and pixel centres at x + 0.5 make u_l = u_0 / 2^l.
                      raw depth float32 d_0 = x for ``source="depth"`` and 1 / (lo + span * x) for ``"disparity"``: the cloud's rule without its last
                                multiply by the gain.  A pixel of level 0 is valid when the cloud keeps it: the mask, and near < z < far with
                                z = d_0 * gain32 at the gain of the guess.  A pixel of a level >= 1 is valid when its stored value is not 0.
                      reduce    float32, every operation rounded on its own.  The block (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1) of level l, in
                                that order:  m = the smallest valid value;  a valid value is used when d <= m * one_plus_jump, with
                                one_plus_jump = float32(1.0 + jump) formed in Python doubles and rounded once;  s = the used values added in block
                                order, starting from the first used one;  c = their count;  the stored value is s / float32(c), or +0 where nothing
                                is valid.  The nearest surface wins, so a block across a depth edge is not smeared; this is also the first
                                depth-jump test the live side gets.  ``jump = inf`` uses every valid value, ``jump = 0`` only those equal to m.
                      colour    RGB level l+1 is per channel (a + b + c + d + 2) >> 2 over the same block, in integers; validity is ignored, as the
                                frames carry none.
                      consuming a level l >= 1 is an ordinary clip for the kernels above: Cloud(K=K_l, pose=T, source="depth", gain=the gain of
                                level 0, near, far, mask=None, step=1) over the stored level, so z = d_l * gain32 and the near/far test drops the
                                zeros.  The gain was kept out of the stored values, so ``set_gain`` of "scale" works unchanged.
                      track     the levels run from L down to 0; with ``pyramid`` set ``iterations`` is not used.  A level with 0 steps is skipped
                                entirely: no ray-cast, no normals.  The two pyramids are formed once per tracked frame, up to the coarsest level
                                that is run.  Entering level l the model is ``raycast(track.views(K_l, T, (h_l, w_l)))`` from the current estimate T
                                (the guess for the first level run).  ``max_dist``, ``min_pairs``, ``min_cos``, ``huber``, ``huber_colour``, ``colour``
                                and the scale's update and bounds apply at every level as they are (a wider ``max_dist`` on coarse levels was tried
                                on the mirror and lost accuracy); the live normals for ``min_cos`` are formed once per level on the level's
                                selection, with the gain of the guess.  A level that loses the frame loses the frame: the guess comes back.
                                ``pairs`` and ``rms`` are those of the last step run;  R is re-orthonormalised once, after the last level.
                      One launch a frame makes all depth levels and one all colour levels (a workgroup per 32 x 32 tile of level 0, which holds
                      whole blocks of every level; levels 2 and up are reduced through LDS); no atomics, every pixel of every level written once.
                      Measured on the mirror (tests/test_track_pyramid_cpu.py) on the scene of tests/track_cases.py, guess the identity,
                      min_pairs = 16: at five times the scene's motion (0.195 rad) the plain tracker with 19 steps ends 6.83e-1 rad / 4.99e-1
                      from the truth, ``pyramid=(10, 5, 4)`` 9.2e-4 / 5.5e-4; at the scene's own motion 9.4e-4 / 4.5e-4 against 7.1e-5 / 1.3e-5.
                      On so small and smooth a scene the gain in reach is modest (4.5 times converges either way, 5.5 times is lost either way,
                      the overlap runs out).  Times on the GPU at 518 x 518 are in DESIGN.md, "Coarse-to-fine tracking": there the coarse plans
                      are slower than six full-size steps, because a ray-cast is bound by the length of a ray and a step by its launches and
                      its host wait, so the option is for reach, not for speed.

What is not built: hashed or sparse volumes, shading, free-space skipping, and in the tracker an affine correction in disparity (scale and shift;
the scale alone is ``Track(scale=True)``), a depth-jump test inside the live normals (the pyramid's ``jump`` tests the blocks it averages, level 0
has none), a model pyramid down-sampled instead of re-cast, a solve on the device, loop closure and relocalisation after a lost frame."""
from __future__ import annotations

import ctypes as C
import dataclasses
import itertools
import math
from dataclasses import KW_ONLY, dataclass

import numpy as np
import torch

from . import _lib
from .cloud import MAX_FRAMES, Cloud, PointCloud, _check_clip, _on_device, selection


def __getattr__(name):
    if name == "TILE_VOXELS":  # voxels per workgroup of the extraction kernels, from the library's own constant
        return int(_lib.load().edv_tsdf_tile_voxels())
    if name == "PYRAMID_MAX_LEVELS":  # the levels of a pyramid, level 0 included: the pyramid kernel's tile is 2^(levels - 1) pixels a side
        return int(_lib.load().edv_pyramid_max_levels())
    raise AttributeError(name)


@dataclass(frozen=True, eq=False)
class Volume:
    origin: object                           # the corner of voxel (0, 0, 0), world units: three floats
    voxel: float                             # edge of a voxel
    dims: object                             # (nx, ny, nz)
    trunc: float = None                      # truncation distance; None = 4 * voxel
    max_weight: float = 64.0                 # the running average forgets beyond this many observations

    def __post_init__(self):
        origin = np.asarray(self.origin, dtype=np.float64)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError(f"origin must be three finite numbers, got {self.origin!r}")
        object.__setattr__(self, "origin", tuple(float(v) for v in origin))
        if not _positive(self.voxel):
            raise ValueError(f"voxel must be finite and positive, got {self.voxel!r}")
        object.__setattr__(self, "voxel", float(self.voxel))
        dims = tuple(self.dims) if np.ndim(self.dims) == 1 else ()
        if len(dims) != 3 or any(isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 1 for d in dims):
            raise ValueError(f"dims must be three integers >= 1, got {self.dims!r}")
        dims = tuple(int(d) for d in dims)
        if dims[0] * dims[1] * dims[2] >= 2 ** 31:
            raise ValueError(f"a volume holds fewer than 2^31 voxels, got {dims}")
        object.__setattr__(self, "dims", dims)
        trunc = 4.0 * self.voxel if self.trunc is None else self.trunc
        if not _positive(trunc):
            raise ValueError(f"trunc must be finite and positive, got {self.trunc!r}")
        object.__setattr__(self, "trunc", float(trunc))
        if not _positive(self.max_weight) or not _positive(float(np.float32(self.max_weight))):
            raise ValueError(f"max_weight must be finite and positive (as float32), got {self.max_weight!r}")
        object.__setattr__(self, "max_weight", float(self.max_weight))

    @property
    def voxels(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    @classmethod
    def bounding(cls, points, voxel, margin=None, trunc=None, max_weight=64.0) -> "Volume":
        """The volume of ``voxel``-sized voxels around host ``points`` [m, 3] with ``margin`` (default: the truncation distance) on every side."""
        p = np.asarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1 or not np.isfinite(p).all():
            raise ValueError(f"points must be finite, [m, 3] with m >= 1; got shape {tuple(p.shape)}")
        if not _positive(voxel):
            raise ValueError(f"voxel must be finite and positive, got {voxel!r}")
        if margin is None:
            margin = 4.0 * float(voxel) if trunc is None else float(trunc)
        if not (isinstance(margin, (int, float, np.floating, np.integer)) and math.isfinite(margin) and margin >= 0.0):
            raise ValueError(f"margin must be finite and >= 0, got {margin!r}")
        lo, hi = p.min(axis=0) - float(margin), p.max(axis=0) + float(margin)
        dims = np.maximum(np.ceil((hi - lo) / float(voxel)), 1.0).astype(np.int64)
        dims += (lo + dims * float(voxel) < hi)  # the division rounded down across an integer
        return cls(origin=lo, voxel=voxel, dims=tuple(int(d) for d in dims), trunc=trunc, max_weight=max_weight)


def _positive(x) -> bool:
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool) and math.isfinite(x) and x > 0.0


def cameras(spec: Cloud, n: int) -> np.ndarray:
    """float64 [1 or n, 18]: per camera rows 0..2 of ``np.linalg.inv`` of the 4x4 T_world_camera, row-major, then K00 K01 K02 K10 K11 K12; one row
    when K and pose are shared by all frames.  Formed once, in float64, and used by the kernels and the mirror alike."""
    for a, what in ((spec.K, "K"), (spec.pose, "pose")):
        if a.shape[0] not in (1, n):
            raise ValueError(f"{what} holds {a.shape[0]} matrices for {n} frames")
    if not (spec.K[:, 2, :] == np.array([0.0, 0.0, 1.0])).all():
        raise ValueError("the last row of K must be [0, 0, 1]")
    m = max(spec.K.shape[0], spec.pose.shape[0])
    T = np.zeros((spec.pose.shape[0], 4, 4))
    T[:, :3, :], T[:, 3, 3] = spec.pose, 1.0
    try:
        inv = np.linalg.inv(T)
    except np.linalg.LinAlgError:
        raise ValueError("pose must be invertible") from None
    W = np.broadcast_to(inv[:, :3, :], (m, 3, 4))
    K = np.broadcast_to(spec.K[:, :2, :], (m, 2, 3))
    return np.ascontiguousarray(np.concatenate([W.reshape(m, 12), K.reshape(m, 6)], axis=1))


def _check_integrate(depth, spec, frames, coloured):
    n, h, w = _check_clip(depth, spec, frames)
    if int(spec.step) != 1:
        raise ValueError(f"fusion samples the full-resolution clip: the Cloud must have step 1, got {spec.step}")
    if not 1 <= n <= MAX_FRAMES:
        raise ValueError(f"1 to {MAX_FRAMES} frames per call, got {n}")
    if h < 1 or w < 1:
        raise ValueError(f"empty frames: {h} x {w}")
    if coloured != (frames is not None):
        raise ValueError("a coloured volume takes frames and an uncoloured one takes none")
    return n, h, w, cameras(spec, n), spec.frame_mask(n, h, w)


def _check_surface(min_weight, output):
    if output not in ("host", "device"):
        raise ValueError(f"output must be 'host' or 'device', got {output!r}")
    if isinstance(min_weight, bool) or not isinstance(min_weight, (int, float, np.floating, np.integer)) or not min_weight >= 0.0 or math.isinf(min_weight):
        raise ValueError(f"min_weight must be finite and >= 0, got {min_weight!r}")
    return np.float32(min_weight)


@dataclass(eq=False)
class Mesh:
    """An indexed triangle mesh: numpy arrays, or tensors on the GPU."""
    vertices: object                         # float32 [V, 3]
    normals: object                          # float32 [V, 3] unit vectors towards free space, or None
    colors: object                           # uint8 [V, 3], or None
    triangles: object                        # int32 [F, 3] vertex indices, counter-clockwise seen from free space


OFFSETS = tuple((d & 1, d >> 1 & 1, d >> 2 & 1) for d in range(8))
TETRAHEDRA = tuple((0, 1 << p, (1 << p) | (1 << q), 7) for p, q, _ in itertools.permutations(range(3)))


def _mesh_table() -> np.ndarray:
    """int8 [6, 16, 2, 3, 2]: per tetrahedron and case mask up to two triangles of three edges (u, d), u the cube corner that owns the edge and
    d = v - u; -1 where there is no triangle.  The rule of the module docstring, in integers: twice the midpoints, and the direction from the
    inside to the outside corners scaled by both counts."""
    table = np.full((6, 16, 2, 3, 2), -1, np.int8)
    for ti, corners in enumerate(TETRAHEDRA):
        P = np.array([OFFSETS[c] for c in corners], np.int64)
        for m in range(1, 15):
            ins, outs = [i for i in range(4) if m >> i & 1], [i for i in range(4) if not m >> i & 1]
            if len(ins) == 1:
                poly = [(ins[0], o) for o in outs]
            elif len(ins) == 3:
                poly = [(i, outs[0]) for i in ins]
            else:
                (a, b), (c, d) = ins, outs
                poly = [(a, c), (a, d), (b, d), (b, c)]
            pts = [P[i] + P[j] for i, j in poly]
            towards = len(ins) * P[outs].sum(axis=0) - len(outs) * P[ins].sum(axis=0)
            if np.cross(pts[1] - pts[0], pts[2] - pts[0]) @ towards < 0:
                poly = poly[::-1]
            for k, tri in enumerate([poly[:3]] if len(poly) == 3 else [poly[:3], [poly[0], poly[2], poly[3]]]):
                for e, (i, j) in enumerate(tri):
                    u, v = sorted((corners[i], corners[j]))
                    table[ti, m, k, e] = (u, v - u)
    return table


MESH_TABLE = _mesh_table()
MESH_TABLE.setflags(write=False)


def _check_mesh(min_weight, normals, output):
    if not isinstance(normals, (bool, np.bool_)):
        raise ValueError(f"normals must be True or False, got {normals!r}")
    return _check_surface(min_weight, output)


MAX_STEPS = 65536  # samples along a ray: the bound of the kernel's loop


@dataclass(frozen=True, eq=False)
class Views:
    """The cameras that look at a volume (module docstring, "views"), and how their rays are sampled."""
    K: object                                # intrinsics [3, 3] or [m, 3, 3]
    pose: object = None                      # T_world_camera [3, 4] / [4, 4] or one per view; None = identity
    _: KW_ONLY
    size: object                             # (h, w) of every view
    near: float                              # the first sample's depth
    far: float                               # no sample lies beyond it
    step: float = None                       # depth between two samples; None = the volume's voxel

    def __post_init__(self):
        spec = Cloud(K=self.K, pose=self.pose)                   # finite, well-formed, K invertible
        counts = (spec.K.shape[0], spec.pose.shape[0])
        if min(counts) != 1 and counts[0] != counts[1]:
            raise ValueError(f"K holds {counts[0]} matrices and pose {counts[1]}: equal counts, or one of them a single matrix")
        object.__setattr__(self, "K", spec.K)
        object.__setattr__(self, "pose", spec.pose)
        size = tuple(self.size) if np.ndim(self.size) == 1 else ()
        if len(size) != 2 or any(isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 1 for d in size):
            raise ValueError(f"size must be two integers (h, w) >= 1, got {self.size!r}")
        object.__setattr__(self, "size", tuple(int(d) for d in size))
        for name in ("near", "far"):
            x = getattr(self, name)
            if isinstance(x, bool) or not isinstance(x, (int, float, np.floating, np.integer)) or not math.isfinite(x):
                raise ValueError(f"{name} must be a finite number, got {x!r}")
            object.__setattr__(self, name, float(x))
        if not 0.0 <= self.near < self.far:
            raise ValueError(f"need 0 <= near < far, got near={self.near!r}, far={self.far!r}")
        if self.step is not None:
            if not _positive(self.step):
                raise ValueError(f"step must be finite and positive, got {self.step!r}")
            object.__setattr__(self, "step", float(self.step))
            self.march(self.step)
        if self.count * self.size[0] * self.size[1] >= 2 ** 31:
            raise ValueError(f"the views hold fewer than 2^31 pixels, got {self.count} x {self.size[0]} x {self.size[1]}")

    @property
    def count(self) -> int:
        return max(self.K.shape[0], self.pose.shape[0])

    def march(self, voxel: float):
        """(step, steps): the depth between two samples (the volume's ``voxel`` unless the views set one) and the number of samples,
        floor((far - near) / step) + 1 in float64."""
        step = float(voxel) if self.step is None else self.step
        steps = math.floor((self.far - self.near) / step) + 1
        if steps > MAX_STEPS:
            raise ValueError(f"step {step!r} gives {steps} samples between near and far, at most {MAX_STEPS}")
        return step, steps

    def cams(self) -> np.ndarray:
        """float64 [m, 21]: ``cloud.Cloud.cams`` of these cameras, one row per view."""
        m = self.count
        return np.ascontiguousarray(np.broadcast_to(Cloud(K=self.K, pose=self.pose).cams(m), (m, 21)))


@dataclass(eq=False)
class Raycast:
    """The fused surface as the views see it: numpy arrays, or tensors on the GPU."""
    depth: object                            # float32 [m, h, w], the cloud's depth of the surface along each pixel's ray; 0 where it finds none
    normals: object                          # float32 [m, h, w, 3] unit vectors in the world frame towards free space, or None
    colors: object                           # uint8 [m, h, w, 3], or None


def _check_raycast(views, min_weight, normals, output):
    if not isinstance(views, Views):
        raise ValueError(f"views must be a fusion.Views, got {type(views).__name__}")
    return _check_mesh(min_weight, normals, output)


def _cell(g, dims):
    """The cells [3, p] int64 that hold the points g [3, p] (voxel-centre coordinates) and the float32 positions inside them."""
    c = np.stack([np.minimum(np.maximum(g[i].astype(np.int64), 0), dims[i] - 2) for i in range(3)])
    return c, (g - c.astype(np.float64)).astype(np.float32)


def _trilinear(q, f):
    """q [8, p, ...] float32 at the corners c = x | y << 1 | z << 2 and f [3, p]: along x, then y, then z, every operation rounded on its own."""
    fx, fy, fz = (f[i].reshape(f[i].shape + (1,) * (q.ndim - 2)) for i in range(3))
    a00, a10 = q[0] + fx * (q[1] - q[0]), q[2] + fx * (q[3] - q[2])
    a01, a11 = q[4] + fx * (q[5] - q[4]), q[6] + fx * (q[7] - q[6])
    b0, b1 = a00 + fy * (a10 - a00), a01 + fy * (a11 - a01)
    return b0 + fz * (b1 - b0)


def _staged(a: np.ndarray, dev: torch.device) -> torch.Tensor:
    """A host array on the GPU through pinned memory, ordered on the current stream: the host does not wait for the stream's earlier work."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).pin_memory().to(dev, non_blocking=True)


# ---- tracking -------------------------------------------------------------------------------------------------------------------------------
ICP_TERMS = 29   # the upper triangle of J J^T (21), J e (6), e e, and the count
ICP_SCALED_TERMS = 37   # with the scale as a seventh column: 28, 7, e e, and the count
_ICP_COLS = {ICP_TERMS: 6, ICP_SCALED_TERMS: 7}
ICP_TILE = 256   # output pixels per tile of the ordered sum: edv_icp_tile_pixels()
_LANE = np.arange(64)


def _number(x) -> bool:
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool) and math.isfinite(x)


@dataclass(frozen=True, eq=False)
class Track:
    """How a frame is tracked against the volume (module docstring, "tracking")."""
    _: KW_ONLY
    near: float                              # the range of the model's ray-cast, as in ``Views``
    far: float
    step: float = None                       # depth between two samples of the ray-cast; None = the volume's voxel
    iterations: int = 6                      # ICP steps per frame
    max_dist: float = None                   # pairs farther apart than this are dropped; None = the volume's trunc
    min_pairs: int = 64                      # fewer pairs than this: the frame is lost
    min_weight: float = 1.0                  # of the ray-cast
    scale: bool = False                      # the frame's depth scale is a seventh unknown (module docstring, "scale")
    max_scale_step: float = 0.25             # with ``scale``: a frame whose scale leaves [1/(1+m), 1+m] times its guess is lost
    colour: float = None                     # lambda, the weight of one intensity unit against one unit of length (module docstring, "colour"); None = geometry alone
    min_cos: float = None                    # pairs whose live normal, turned by the estimate, has a cosine below this with the model's are dropped (module docstring, "robust"); None = no test
    huber: float = None                      # the Huber threshold of the point-to-plane residual, a length; None = plain least squares
    huber_colour: float = None               # the same for the intensity residual, in levels of 255; needs ``colour``
    pyramid: tuple = None                    # ICP steps per level, finest first (module docstring, "pyramid"); ``iterations`` is then not used.  None = one resolution
    jump: float = 0.05                       # of the depth pyramid: a block averages the valid depths within (1 + jump) of its nearest; inf = all of them

    def __post_init__(self):
        if self.pyramid is not None:
            steps = tuple(self.pyramid) if np.ndim(self.pyramid) == 1 else ()
            if not steps or any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) or i < 0 for i in steps) or not any(i > 0 for i in steps):
                raise ValueError(f"pyramid must be None or the steps per level, integers >= 0 with one > 0, finest first; got {self.pyramid!r}")
            if len(steps) > int(_lib.load().edv_pyramid_max_levels()):
                raise ValueError(f"a pyramid has at most {int(_lib.load().edv_pyramid_max_levels())} levels (PYRAMID_MAX_LEVELS), got {len(steps)}")
            object.__setattr__(self, "pyramid", tuple(int(i) for i in steps))
        _one_plus_jump(self.jump)
        object.__setattr__(self, "jump", float(self.jump))
        if self.colour is not None:
            if not _positive(self.colour):
                raise ValueError(f"colour must be None or finite and positive, got {self.colour!r}")
            object.__setattr__(self, "colour", float(self.colour))
        if self.min_cos is not None:
            if not _number(self.min_cos) or not -1.0 <= self.min_cos <= 1.0:
                raise ValueError(f"min_cos must be None or a number in [-1, 1], got {self.min_cos!r}")
            object.__setattr__(self, "min_cos", float(self.min_cos))
        for name in ("huber", "huber_colour"):
            x = getattr(self, name)
            if x is not None:
                if not _positive(x):
                    raise ValueError(f"{name} must be None or finite and positive, got {x!r}")
                object.__setattr__(self, name, float(x))
        if self.huber_colour is not None and self.colour is None:
            raise ValueError("huber_colour weighs the colour residual: it needs colour")
        if not isinstance(self.scale, bool):
            raise ValueError(f"scale must be True or False, got {self.scale!r}")
        if not _positive(self.max_scale_step):
            raise ValueError(f"max_scale_step must be finite and positive, got {self.max_scale_step!r}")
        object.__setattr__(self, "max_scale_step", float(self.max_scale_step))
        for name in ("near", "far"):
            if not _number(getattr(self, name)):
                raise ValueError(f"{name} must be a finite number, got {getattr(self, name)!r}")
            object.__setattr__(self, name, float(getattr(self, name)))
        if not 0.0 <= self.near < self.far:
            raise ValueError(f"need 0 <= near < far, got near={self.near!r}, far={self.far!r}")
        for name in ("step", "max_dist"):
            x = getattr(self, name)
            if x is not None:
                if not _positive(x):
                    raise ValueError(f"{name} must be finite and positive, got {x!r}")
                object.__setattr__(self, name, float(x))
        for name in ("iterations", "min_pairs"):
            x = getattr(self, name)
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
                raise ValueError(f"{name} must be an integer >= 1, got {x!r}")
            object.__setattr__(self, name, int(x))
        _check_surface(self.min_weight, "host")
        object.__setattr__(self, "min_weight", float(self.min_weight))

    def views(self, K, pose, size) -> Views:
        """The one view the model is cast from."""
        return Views(K, pose, size=size, near=self.near, far=self.far, step=self.step)

    def robust(self) -> dict:
        """The options of the robust sums that are set; empty: the plain kernels."""
        return {k: v for k, v in (("min_cos", self.min_cos), ("huber", self.huber), ("huber_colour", self.huber_colour)) if v is not None}


@dataclass(eq=False)
class Tracked:
    """What ``track_clip`` found, per frame; numpy arrays on the host."""
    poses: np.ndarray                        # float64 [n, 4, 4] T_world_camera; a lost frame repeats the previous pose
    pairs: np.ndarray                        # int64 [n], the pairs of the last ICP step; 0 for frame 0
    rms: np.ndarray                          # float64 [n], the root mean square point-to-plane distance of those pairs; 0 for frame 0
    lost: np.ndarray                         # bool [n]; a lost frame is not integrated
    scales: np.ndarray = None                # float64 [n] with ``Track(scale=True)``: sigma_i relative to ``spec.gain``, 1.0 for frame 0; a lost frame repeats the previous one.  None otherwise


def _check_icp(depth, spec, model, views, max_dist, frame, frames=None):
    """(n, h, w, mask, cams [1 or n, 21], the model's 39 doubles) of checked arguments; with ``frames`` the model must carry colours."""
    n, h, w = _check_clip(depth, spec, frames)
    if not 1 <= n <= MAX_FRAMES or h < 1 or w < 1:
        raise ValueError(f"1 to {MAX_FRAMES} frames that are not empty, got {n} x {h} x {w}")
    if isinstance(frame, bool) or not isinstance(frame, (int, np.integer)) or not 0 <= frame < n:
        raise ValueError(f"frame must be an integer in 0 .. {n - 1}, got {frame!r}")
    if not isinstance(views, Views) or views.count != 1:
        raise ValueError("views must be a fusion.Views of one view, the one the model was cast from")
    if not isinstance(model, Raycast) or model.normals is None:
        raise ValueError("model must be a fusion.Raycast with normals")
    mh, mw = views.size
    if frames is not None:
        a = model.colors
        if a is None or tuple(a.shape) != (1, mh, mw, 3) or str(a.dtype).replace("torch.", "") != "uint8":
            raise ValueError(f"expected the model's colors as uint8 {[1, mh, mw, 3]}, got {None if a is None else (a.dtype, tuple(a.shape))}")
    for a, shape, what in ((model.depth, (1, mh, mw), "depth"), (model.normals, (1, mh, mw, 3), "normals")):
        if tuple(a.shape) != shape or str(a.dtype).replace("torch.", "") != "float32":
            raise ValueError(f"expected the model's {what} as float32 {list(shape)}, got {a.dtype} {tuple(a.shape)}")
    if not _number(max_dist) or max_dist < 0.0:
        raise ValueError(f"max_dist must be finite and >= 0, got {max_dist!r}")
    model_cam = np.concatenate([views.cams()[0], cameras(Cloud(K=views.K, pose=views.pose), 1)[0]])
    return n, h, w, spec.frame_mask(n, h, w), spec.cams(n), model_cam


def _pose4(pose34) -> np.ndarray:
    T = np.eye(4)
    T[:3, :] = pose34
    return T


def _live_cam(kinv9, T) -> np.ndarray:
    """The row of ``Cloud.cams`` of the pose T with the inverse intrinsics kinv9."""
    return np.concatenate([kinv9, T[:3, :3].reshape(9), T[:3, 3]])


def _ordered_sum(terms: np.ndarray) -> np.ndarray:
    """float64 [p, 29] (or [p, 37]) per output pixel in row-major order -> [29] (or [37]), added in the kernel's order: tiles of 256 pixels, a wave 64 of them; a
    butterfly inside the wave, the four waves in order, then the tiles in order, starting from tile 0's value."""
    p = terms.shape[0]
    tiles = -(-p // ICP_TILE)
    count = terms.shape[1]
    x = np.zeros((tiles * ICP_TILE, count))
    x[:p] = terms
    x = x.reshape(tiles, ICP_TILE // 64, 64, count)
    for s in (32, 16, 8, 4, 2, 1):
        x = x + x[:, :, _LANE ^ s, :]
    wave = x[:, :, 0, :]
    tile = ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]
    total = tile[0].copy()
    for b in range(1, tiles):
        total = total + tile[b]
    return total


def _intensity(rgb: np.ndarray) -> np.ndarray:
    """float64 [...]: (0.299*R + 0.587*G) + 0.114*B of uint8 [..., 3], every operation rounded on its own."""
    c = rgb.astype(np.float64)
    return (0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]


def _depth_rule(x: np.ndarray, source: str, scalars, gain):
    """(z float32, kept) of float32 ``x`` for the float32 ``gain``: the cloud's depth rule with the ``Cloud.scalars()`` given."""
    lo, span, _, near, far = scalars
    gain = np.float32(gain)
    with np.errstate(all="ignore"):
        if source == "depth":
            z = x * gain
        else:
            scaled = lo + span * x
            z = np.float32(1.0) / scaled
            z = z * gain
        keep = (z > near) & (z < far)
    return z, keep


def _grid_samples(h: int, w: int, step: int):
    """The source rows and columns of the cloud's output grid."""
    oh, ow = -(-h // step), -(-w // step)
    return np.minimum(np.arange(oh, dtype=np.int64) * step + step // 2, h - 1), np.minimum(np.arange(ow, dtype=np.int64) * step + step // 2, w - 1)


def _grid_normals(z: np.ndarray, keep: np.ndarray, kinv: np.ndarray, step: int) -> np.ndarray:
    """float32 [oh, ow, 3]: the live normals (module docstring, "robust") of one frame's output grid from its z (float32) and kept."""
    oh, ow = z.shape
    out = np.zeros((oh, ow, 3), np.float32)
    if oh < 3 or ow < 3:
        return out
    u = ((np.arange(ow, dtype=np.float64) + 0.5) * float(step))[None, :]
    v = ((np.arange(oh, dtype=np.float64) + 0.5) * float(step))[:, None]
    with np.errstate(all="ignore"):
        zz = z.astype(np.float64)
        V = [((kinv[i, 0] * u + kinv[i, 1] * v) + kinv[i, 2]) * zz for i in range(3)]
        a = [V[i][1:-1, 2:] - V[i][1:-1, :-2] for i in range(3)]
        b = [V[i][2:, 1:-1] - V[i][:-2, 1:-1] for i in range(3)]
        c = [b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]]
        length = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        valid = keep[1:-1, 1:-1] & keep[1:-1, 2:] & keep[1:-1, :-2] & keep[2:, 1:-1] & keep[:-2, 1:-1] & (length > 0.0)
        for i in range(3):
            out[1:-1, 1:-1, i] = np.where(valid, c[i] / length, 0.0).astype(np.float32)
    return out


def _check_normals(depth, spec):
    n, h, w = _check_clip(depth, spec, None)
    if not 1 <= n <= MAX_FRAMES or h < 1 or w < 1:
        raise ValueError(f"1 to {MAX_FRAMES} frames that are not empty, got {n} x {h} x {w}")
    return n, h, w, spec.frame_mask(n, h, w), spec.cams(n)


def frame_normals_host(depth, spec: Cloud) -> np.ndarray:
    """``frame_normals`` in numpy, the same operations in the same order: the two agree bit for bit."""
    depth = np.asarray(depth)
    n, h, w, mask, cams = _check_normals(depth, spec)
    step = int(spec.step)
    sy, sx = _grid_samples(h, w, step)
    scalars = spec.scalars()
    out = np.empty((n, sy.shape[0], sx.shape[0], 3), np.float32)
    for f in range(n):
        z, keep = _depth_rule(depth[f][sy][:, sx], spec.source, scalars, scalars[2])
        if mask is not None:
            keep &= (mask[f] if mask.ndim == 3 else mask)[sy][:, sx] != 0
        out[f] = _grid_normals(z, keep, cams[f if cams.shape[0] > 1 else 0, :9].reshape(3, 3), step)
    return out


def _frame_normals_device(lib, sel, cams_d: torch.Tensor, first: int, count: int, device) -> torch.Tensor:
    """``edv_frame_normals`` of frames first .. first + count - 1 of the selection ``sel`` on the current stream: float32 [count, oh, ow, 3] on the GPU."""
    step = int(sel.step)
    out = torch.empty((count, -(-int(sel.h) // step), -(-int(sel.w) // step), 3), dtype=torch.float32, device=device)
    _lib.check(lib.edv_frame_normals(C.byref(sel), cams_d.data_ptr(), 21 if cams_d.shape[0] > 1 else 0, first, count, out.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "edv_frame_normals")
    return out


def frame_normals(depth, spec: Cloud, output: str = "host"):
    """float32 [n, oh, ow, 3]: the normal of every pixel of the cloud's output grid in its camera's frame (module docstring, "robust"), from central
    differences of the clip's own vertices; (0, 0, 0) where the pixel or one of its four neighbours is not kept, and on the grid's border.
    ``depth`` is float32 [n, h, w], a numpy array or a tensor on the GPU; the pose of ``spec`` is not looked at.  On the GPU, on the caller's
    current stream: a numpy array, complete when returned, or with ``output="device"`` a tensor ordered on that stream."""
    if output not in ("host", "device"):
        raise ValueError(f"output must be 'host' or 'device', got {output!r}")
    if isinstance(depth, torch.Tensor):
        if not depth.is_cuda:
            raise ValueError("a depth tensor must live on the GPU (pass host data as a numpy array)")
        device = depth.device
    else:
        depth, device = np.asarray(depth), torch.device("cuda", torch.cuda.current_device())
    n, h, w, mask, cams = _check_normals(depth, spec)
    with torch.cuda.device(device):
        x = _on_device(depth, device)
        mask_d = None if mask is None else _staged(mask, device)
        out = _frame_normals_device(_lib.load(), selection(x, spec, mask_d), _staged(cams, device), 0, n, device)
        if output == "device":
            return out
        host = torch.empty(out.shape, dtype=torch.float32, pin_memory=True)
        host.copy_(out, non_blocking=True)
        torch.cuda.current_stream(device).synchronize()
        return host.numpy().copy()


def _one_plus_jump(jump) -> np.float32:
    """1 + jump as the float32 both implementations compare with: formed in Python doubles and rounded once."""
    if isinstance(jump, bool) or not isinstance(jump, (int, float, np.floating, np.integer)) or not jump >= 0.0:
        raise ValueError(f"jump must be a number >= 0 (inf: every valid depth of a block is used), got {jump!r}")
    return np.float32(1.0 + float(jump))


def _pyramid_sizes(h: int, w: int, levels) -> list:
    """[(h_l, w_l) for l = 1 .. levels]: each level half the one below, an odd last row or column dropped."""
    most = int(_lib.load().edv_pyramid_max_levels()) - 1
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= levels <= most:
        raise ValueError(f"levels must be an integer in 1 .. {most} (PYRAMID_MAX_LEVELS - 1), got {levels!r}")
    sizes = []
    for l in range(1, int(levels) + 1):
        h, w = h // 2, w // 2
        if h < 1 or w < 1:
            raise ValueError(f"level {l} of the pyramid holds no pixel")
        sizes.append((h, w))
    return sizes


def _check_level0(spec: Cloud) -> None:
    """What the depth pyramid needs of the Cloud: a stored +0 must mean "not valid" at every level."""
    if int(spec.step) != 1:
        raise ValueError(f"level 0 of the pyramid is the full-resolution frame: the Cloud must have step 1, got {spec.step}")
    _, _, gain, near, _ = spec.scalars()
    if not near >= 0.0 or not gain > 0.0:
        raise ValueError(f"the pyramid needs near >= 0 and gain > 0 (as float32), got near={spec.near!r}, gain={spec.gain!r}")


def _check_pyramid(depth, spec, levels, jump, frame):
    n, h, w = _check_clip(depth, spec, None)
    if not 1 <= n <= MAX_FRAMES or h < 1 or w < 1:
        raise ValueError(f"1 to {MAX_FRAMES} frames that are not empty, got {n} x {h} x {w}")
    if isinstance(frame, bool) or not isinstance(frame, (int, np.integer)) or not 0 <= frame < n:
        raise ValueError(f"frame must be an integer in 0 .. {n - 1}, got {frame!r}")
    _check_level0(spec)
    return n, h, w, _pyramid_sizes(h, w, levels), _one_plus_jump(jump), spec.frame_mask(n, h, w)


def _check_rgb_pyramid(frames, levels, frame):
    if frames.ndim != 4 or frames.shape[3] != 3 or str(frames.dtype).replace("torch.", "") != "uint8":
        raise ValueError(f"expected uint8 frames [n, h, w, 3], got {frames.dtype} {tuple(frames.shape)}")
    n, h, w = (int(v) for v in frames.shape[:3])
    if n < 1 or h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError(f"frames that are not empty and hold fewer than 2^31 pixels each, got {n} x {h} x {w}")
    if isinstance(frame, bool) or not isinstance(frame, (int, np.integer)) or not 0 <= frame < n:
        raise ValueError(f"frame must be an integer in 0 .. {n - 1}, got {frame!r}")
    return n, h, w, _pyramid_sizes(h, w, levels)


def _blocks(a: np.ndarray):
    """The four pixels of every 2 x 2 block of a [h, w, ...] in block order: (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1)."""
    h, w = a.shape[0] // 2, a.shape[1] // 2
    return [a[i:2 * h:2, j:2 * w:2] for i in (0, 1) for j in (0, 1)]


def _reduce_depth(d: np.ndarray, one_plus_jump: np.float32) -> np.ndarray:
    """Level l+1 of the float32 level ``d`` whose +0 means "not valid" (module docstring, "pyramid")."""
    block = _blocks(d)
    valid = [b != 0 for b in block]
    zero, one = np.float32(0.0), np.float32(1.0)
    with np.errstate(all="ignore"):
        m = np.full(block[0].shape, np.inf, np.float32)
        for b, v in zip(block, valid):
            m = np.where(v, np.minimum(m, b), m)
        limit = m * one_plus_jump
        s, c = np.zeros(m.shape, np.float32), np.zeros(m.shape, np.float32)
        for b, v in zip(block, valid):
            used = v & (b <= limit)
            s, c = np.where(used, s + b, s), np.where(used, c + one, c)     # +0 + d == d: the sum starts from the first used value
        return np.where(c > zero, s / c, zero).astype(np.float32)


def depth_pyramid_host(depth, spec: Cloud, levels: int, jump: float = 0.05, frame: int = 0) -> list:
    """``depth_pyramid`` in numpy, the same operations in the same order: the two agree bit for bit."""
    depth = np.asarray(depth)
    n, h, w, sizes, one_plus_jump, mask = _check_pyramid(depth, spec, levels, jump, frame)
    lo, span, gain, near, far = spec.scalars()
    x = depth[frame]
    with np.errstate(all="ignore"):
        d = x if spec.source == "depth" else np.float32(1.0) / (lo + span * x)
        z = d * gain
        keep = (z > near) & (z < far)
    if mask is not None:
        keep &= (mask[frame] if mask.ndim == 3 else mask) != 0
    d = np.where(keep, d, np.float32(0.0)).astype(np.float32)
    out = []
    for _ in sizes:
        d = _reduce_depth(d, one_plus_jump)
        out.append(d)
    return out


def rgb_pyramid_host(frames, levels: int, frame: int = 0) -> list:
    """``rgb_pyramid`` in numpy: the two agree in every byte."""
    frames = np.asarray(frames)
    n, h, w, sizes = _check_rgb_pyramid(frames, levels, frame)
    c = frames[frame]
    out = []
    for _ in sizes:
        a = [b.astype(np.uint16) for b in _blocks(c)]
        c = ((((a[0] + a[1]) + a[2]) + a[3] + np.uint16(2)) >> np.uint16(2)).astype(np.uint8)
        out.append(c)
    return out


def _pyramid_layout(lib, h: int, w: int, levels: int):
    """(the pixels of levels 1 .. levels together, the pixels in front of each): ``edv_pyramid_pixels``."""
    offsets = (C.c_int64 * levels)()
    total = int(lib.edv_pyramid_pixels(h, w, levels, offsets))
    if total < 1:
        raise ValueError(f"no pyramid of {levels} levels over {h} x {w}")
    return total, [int(o) for o in offsets]


def _depth_pyramid_device(lib, sel, frame: int, sizes, one_plus_jump, device):
    """``edv_depth_pyramid`` of one frame of the selection on the current stream: (the buffer, float32 views [h_l, w_l] of its levels) on the GPU."""
    total, offsets = _pyramid_layout(lib, int(sel.h), int(sel.w), len(sizes))
    buf = torch.empty(total, dtype=torch.float32, device=device)
    _lib.check(lib.edv_depth_pyramid(C.byref(sel), frame, len(sizes), float(one_plus_jump), buf.data_ptr(), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)),
               "edv_depth_pyramid")
    return buf, [buf[o:o + h * w].view(h, w) for o, (h, w) in zip(offsets, sizes)]


def _rgb_pyramid_device(lib, rgb: torch.Tensor, frame: int, sizes, device):
    """``edv_rgb_pyramid`` of one frame of the contiguous uint8 tensor [n, h, w, 3] on the current stream: (the buffer, uint8 views [h_l, w_l, 3])."""
    n, h, w = (int(v) for v in rgb.shape[:3])
    total, offsets = _pyramid_layout(lib, h, w, len(sizes))
    buf = torch.empty(3 * total, dtype=torch.uint8, device=device)
    _lib.check(lib.edv_rgb_pyramid(rgb.data_ptr(), n, h, w, frame, len(sizes), buf.data_ptr(), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "edv_rgb_pyramid")
    return buf, [buf[3 * o:3 * (o + lh * lw)].view(lh, lw, 3) for o, (lh, lw) in zip(offsets, sizes)]


def _levels_out(buf: torch.Tensor, levels: list, output: str, device):
    """The levels as they are (tensors, ordered on the current stream) or as numpy arrays: one copy of the buffer, for which the host waits."""
    if output == "device":
        return levels
    host = torch.empty(buf.shape, dtype=buf.dtype, pin_memory=True)
    host.copy_(buf, non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    flat, out, at = host.numpy(), [], 0
    for l in levels:
        out.append(flat[at:at + l.numel()].reshape(tuple(l.shape)).copy())
        at += l.numel()
    return out


def depth_pyramid(depth, spec: Cloud, levels: int, jump: float = 0.05, frame: int = 0, output: str = "host") -> list:
    """Levels 1 .. ``levels`` of the depth pyramid of frame ``frame`` (module docstring, "pyramid"): a list of float32 [h_l, w_l], the raw depth
    (the cloud's depth without its gain) averaged over 2 x 2 blocks, the nearest surface of a block alone, +0 where nothing is valid.
    ``depth`` is float32 [n, h, w], a numpy array or a tensor on the GPU; ``spec`` needs step 1, near >= 0 and gain > 0, its K and pose are not
    looked at.  One launch (``edv_depth_pyramid``) on the caller's current stream: numpy arrays, complete when returned, or with
    ``output="device"`` tensors ordered on that stream."""
    if output not in ("host", "device"):
        raise ValueError(f"output must be 'host' or 'device', got {output!r}")
    if isinstance(depth, torch.Tensor):
        if not depth.is_cuda:
            raise ValueError("a depth tensor must live on the GPU (pass host data as a numpy array)")
        device = depth.device
    else:
        depth, device = np.asarray(depth), torch.device("cuda", torch.cuda.current_device())
    n, h, w, sizes, one_plus_jump, mask = _check_pyramid(depth, spec, levels, jump, frame)
    with torch.cuda.device(device):
        x = _on_device(depth, device)
        mask_d = None if mask is None else _staged(mask, device)
        buf, out = _depth_pyramid_device(_lib.load(), selection(x, spec, mask_d), int(frame), sizes, one_plus_jump, device)
        return _levels_out(buf, out, output, device)


def rgb_pyramid(frames, levels: int, frame: int = 0, output: str = "host") -> list:
    """Levels 1 .. ``levels`` of the colour pyramid of frame ``frame`` of ``frames`` (uint8 [n, h, w, 3], an array or a tensor on the GPU): a list of
    uint8 [h_l, w_l, 3], per channel (a + b + c + d + 2) >> 2 over the depth pyramid's blocks.  One launch (``edv_rgb_pyramid``) on the caller's
    current stream; ``output`` as for ``depth_pyramid``."""
    if output not in ("host", "device"):
        raise ValueError(f"output must be 'host' or 'device', got {output!r}")
    if isinstance(frames, torch.Tensor):
        if not frames.is_cuda:
            raise ValueError("a frames tensor must live on the GPU (pass host data as a numpy array)")
        device = frames.device
    else:
        frames, device = np.asarray(frames), torch.device("cuda", torch.cuda.current_device())
    n, h, w, sizes = _check_rgb_pyramid(frames, levels, frame)
    with torch.cuda.device(device):
        buf, out = _rgb_pyramid_device(_lib.load(), _on_device(frames, device), int(frame), sizes, device)
        return _levels_out(buf, out, output, device)


def _check_robust(colour: bool, min_cos=None, huber=None, huber_colour=None):
    """(min_cos or None, huber, huber_colour) of checked options of the robust sums; a threshold that is not given is +inf."""
    if min_cos is not None and (not _number(min_cos) or not -1.0 <= min_cos <= 1.0):
        raise ValueError(f"min_cos must be None or a number in [-1, 1], got {min_cos!r}")
    for name, x in (("huber", huber), ("huber_colour", huber_colour)):
        if x is not None and (isinstance(x, bool) or not isinstance(x, (int, float, np.floating, np.integer)) or not x > 0.0):
            raise ValueError(f"{name} must be None or positive (inf: no weight), got {x!r}")
    if huber_colour is not None and not colour:
        raise ValueError("huber_colour weighs the colour residual: it needs the frames and a model with colours")
    return None if min_cos is None else float(min_cos), math.inf if huber is None else float(huber), math.inf if huber_colour is None else float(huber_colour)


class _IcpHost:
    """One live frame against one model view in numpy: what does not depend on the estimate is formed once.  ``robust``: None for the plain sums, or
    the options of ``_check_robust`` by name (all of them optional) for the robust ones; the live normals are then formed here, once."""
    output = "host"

    def __init__(self, depth, spec, model, views, max_dist, frame, scale=False, frames=None, robust=None):
        depth = np.asarray(depth)
        frames = None if frames is None else np.asarray(frames)
        n, h, w, mask, cams, self.model_cam = _check_icp(depth, spec, model, views, max_dist, frame, frames)
        self.robust = None if robust is None else _check_robust(frames is not None, **robust)
        self.cols = 7 if scale else 6
        self.kinv = cams[frame if cams.shape[0] > 1 else 0, :9]
        self.max_dist2 = float(max_dist) * float(max_dist)
        step = int(spec.step)
        sy, sx = _grid_samples(h, w, step)
        oh, ow = sy.shape[0], sx.shape[0]
        self.source, self.scalars = spec.source, spec.scalars()
        self.x = depth[frame][sy][:, sx]
        self.unmasked = None if mask is None else (mask[frame] if mask.ndim == 3 else mask)[sy][:, sx] != 0
        self.set_gain(self.scalars[2])
        self.live_normals = None
        if self.robust is not None and self.robust[0] is not None:         # with the gain of the spec, and not again when ``set_gain`` changes it
            self.live_normals = _grid_normals(self.z32, self.keep.reshape(oh, ow), self.kinv.reshape(3, 3), step).astype(np.float64).reshape(-1, 3)
        self.u = np.broadcast_to(((np.arange(ow, dtype=np.float64) + 0.5) * float(step))[None, :], (oh, ow)).reshape(-1)
        self.v = np.broadcast_to(((np.arange(oh, dtype=np.float64) + 0.5) * float(step))[:, None], (oh, ow)).reshape(-1)
        self.depth, self.normals = np.asarray(model.depth)[0], np.asarray(model.normals)[0]
        self.colour = frames is not None
        if self.colour:                                                  # the intensities of the live grid and of the model view, formed once
            self.live_y = _intensity(frames[frame][sy][:, sx]).reshape(-1)
            self.model_y = _intensity(np.asarray(model.colors)[0])

    def set_gain(self, gain) -> None:
        """z and kept of the frame again, in float32, for the float32 ``gain``: the cloud's depth rule."""
        self.z32, keep = _depth_rule(self.x, self.source, self.scalars, gain)
        if self.unmasked is not None:
            keep &= self.unmasked
        self.z, self.keep = self.z32.astype(np.float64).reshape(-1), keep.reshape(-1)

    def terms(self, live: np.ndarray) -> np.ndarray:
        """float64 [oh * ow, 29 or 37]: the terms of every output pixel for the estimate ``live`` (21 doubles), +0 where there is no pair.  With
        colour twice as many: the colour block behind the geometric one."""
        kinv, rot, pos = live[:9].reshape(3, 3), live[9:18].reshape(3, 3), live[18:]
        m = self.model_cam
        kinv_m, rot_m, pos_m, W, K = m[:9].reshape(3, 3), m[9:18].reshape(3, 3), m[18:21], m[21:33].reshape(3, 4), m[33:].reshape(2, 3)
        mh, mw = self.depth.shape
        u, v, z = self.u, self.v, self.z
        with np.errstate(all="ignore"):
            l = [(kinv[i, 0] * u + kinv[i, 1] * v) + kinv[i, 2] for i in range(3)]
            r = [(rot[i, 0] * l[0] + rot[i, 1] * l[1]) + rot[i, 2] * l[2] for i in range(3)]
            rho = [r[i] * z for i in range(3)]
            P = [pos[i] + rho[i] for i in range(3)]
            q = [((W[i, 0] * P[0] + W[i, 1] * P[1]) + W[i, 2] * P[2]) + W[i, 3] for i in range(3)]
            ok = self.keep & (q[2] > 0.0)
            um = ((K[0, 0] * q[0] + K[0, 1] * q[1]) + K[0, 2] * q[2]) / q[2]
            vm = ((K[1, 0] * q[0] + K[1, 1] * q[1]) + K[1, 2] * q[2]) / q[2]
            ok &= (um >= 0.0) & (um < float(mw)) & (vm >= 0.0) & (vm < float(mh))
            px, py = np.where(ok, um, 0.0).astype(np.int64), np.where(ok, vm, 0.0).astype(np.int64)
            dm = self.depth[py, px]
            ok &= dm > 0
            N = [self.normals[py, px, i].astype(np.float64) for i in range(3)]
            ok &= (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2] > 0.0
            mu, mv = px.astype(np.float64) + 0.5, py.astype(np.float64) + 0.5
            lm = [(kinv_m[i, 0] * mu + kinv_m[i, 1] * mv) + kinv_m[i, 2] for i in range(3)]
            rm = [(rot_m[i, 0] * lm[0] + rot_m[i, 1] * lm[1]) + rot_m[i, 2] * lm[2] for i in range(3)]
            D = [(pos_m[i] + rm[i] * dm.astype(np.float64)) - P[i] for i in range(3)]
            ok &= (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2] <= self.max_dist2
            e = (N[0] * D[0] + N[1] * D[1]) + N[2] * D[2]
            J = [rho[1] * N[2] - rho[2] * N[1], rho[2] * N[0] - rho[0] * N[2], rho[0] * N[1] - rho[1] * N[0], N[0], N[1], N[2]]
            if self.cols == 7:
                J.append((rho[0] * N[0] + rho[1] * N[1]) + rho[2] * N[2])
            m = self.cols
            Jw = J
            if self.robust is not None:
                min_cos, huber, huber_colour = self.robust
                if self.live_normals is not None:
                    nl = [self.live_normals[:, i] for i in range(3)]
                    has = (nl[0] * nl[0] + nl[1] * nl[1]) + nl[2] * nl[2] > 0.0
                    nw = [(rot[i, 0] * nl[0] + rot[i, 1] * nl[1]) + rot[i, 2] * nl[2] for i in range(3)]
                    ok &= has & ((N[0] * nw[0] + N[1] * nw[1]) + N[2] * nw[2] >= min_cos)
                weight = np.where(np.abs(e) <= huber, 1.0, huber / np.abs(e))
                Jw = [weight * j for j in J]
            cols = [Jw[j] * J[k] for j in range(m) for k in range(j, m)] + [Jw[j] * e for j in range(m)] + [e * e, np.ones_like(e)]
            cols = [np.where(ok, c, 0.0) for c in cols]
            if self.colour:
                gu, gv = um - 0.5, vm - 0.5
                ok = ok & (mw >= 2) & (mh >= 2) & (gu >= 0.0) & (gu <= float(mw - 1)) & (gv >= 0.0) & (gv <= float(mh - 1))
                x0 = np.minimum(np.where(ok, gu, 0.0).astype(np.int64), max(mw - 2, 0))
                y0 = np.minimum(np.where(ok, gv, 0.0).astype(np.int64), max(mh - 2, 0))
                x1, y1 = np.minimum(x0 + 1, mw - 1), np.minimum(y0 + 1, mh - 1)      # x0 + 1 and y0 + 1 wherever ok can hold
                fx, fy = gu - x0.astype(np.float64), gv - y0.astype(np.float64)
                ok &= (self.depth[y0, x0] > 0) & (self.depth[y0, x1] > 0) & (self.depth[y1, x0] > 0) & (self.depth[y1, x1] > 0)
                Y = self.model_y
                I00, I10, I01, I11 = Y[y0, x0], Y[y0, x1], Y[y1, x0], Y[y1, x1]
                top, bot = I00 + fx * (I10 - I00), I01 + fx * (I11 - I01)
                Im = top + fy * (bot - top)
                Iu = (I10 - I00) + fy * ((I11 - I01) - (I10 - I00))
                Iv = (I01 - I00) + fx * ((I11 - I10) - (I01 - I00))
                a, b = K[0, 0] * q[0] + K[0, 1] * q[1], K[1, 0] * q[0] + K[1, 1] * q[1]
                gq = [(Iu * K[0, 0] + Iv * K[1, 0]) / q[2], (Iu * K[0, 1] + Iv * K[1, 1]) / q[2], -((Iu * a + Iv * b) / (q[2] * q[2]))]
                g = [(W[0, j] * gq[0] + W[1, j] * gq[1]) + W[2, j] * gq[2] for j in range(3)]
                r = self.live_y - Im
                J = [rho[1] * g[2] - rho[2] * g[1], rho[2] * g[0] - rho[0] * g[2], rho[0] * g[1] - rho[1] * g[0], g[0], g[1], g[2]]
                if self.cols == 7:
                    J.append((rho[0] * g[0] + rho[1] * g[1]) + rho[2] * g[2])
                Jw = J
                if self.robust is not None:
                    weight = np.where(np.abs(r) <= huber_colour, 1.0, huber_colour / np.abs(r))
                    Jw = [weight * j for j in J]
                more = [Jw[j] * J[k] for j in range(m) for k in range(j, m)] + [Jw[j] * r for j in range(m)] + [r * r, np.ones_like(r)]
                cols += [np.where(ok, c, 0.0) for c in more]
            return np.stack(cols, axis=1)

    def sums(self, live: np.ndarray) -> np.ndarray:
        return _ordered_sum(self.terms(live))

    @staticmethod
    def placed(depth, frames):
        """The clip and its frames where the sums read them: here, as they are."""
        return depth, frames

    @staticmethod
    def pyramid(depth, spec, frame, levels, jump, frames):
        """(the depth levels 1 .. ``levels`` of the frame as clips [1, h_l, w_l], its colour levels [1, h_l, w_l, 3] or None without ``frames``)."""
        return ([d[None] for d in depth_pyramid_host(depth, spec, levels, jump, frame)],
                None if frames is None else [c[None] for c in rgb_pyramid_host(frames, levels, frame)])


class _IcpDevice:
    """The same on the GPU (``edv_icp_sums``, or ``edv_icp_scaled_sums`` with ``scale``): the clip, the mask, the model and the workspace are
    placed once, an estimate costs two launches and one read of 232 (296) bytes, for which the host waits.  With ``frames``
    (``edv_icp_colour_sums``) the frames and the model's colours are placed once too, and the read is of 464 (592) bytes.  With ``robust`` (as for
    ``_IcpHost``; ``edv_icp_robust_sums``) the frame's normal map is formed once too (``edv_frame_normals``, one more launch) and stays on the GPU."""
    output = "device"

    def __init__(self, depth, spec, model, views, max_dist, frame, device=None, scale=False, frames=None, robust=None):
        if isinstance(depth, torch.Tensor):
            if not depth.is_cuda:
                raise ValueError("a depth tensor must live on the GPU (pass host data as a numpy array)")
            device = depth.device
        else:
            depth = np.asarray(depth)
        if frames is not None and not isinstance(frames, torch.Tensor):
            frames = np.asarray(frames)
        n, h, w, mask, cams, model_cam = _check_icp(depth, spec, model, views, max_dist, frame, frames)
        if device is None:
            device = model.depth.device if isinstance(model.depth, torch.Tensor) and model.depth.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device, self.frame, self.lib = device, int(frame), _lib.load()
        self.colour, self.cols = frames is not None, 7 if scale else 6
        self.name = "edv_icp_colour_sums" if self.colour else "edv_icp_scaled_sums" if scale else "edv_icp_sums"
        self.entry, workspace = getattr(self.lib, self.name), self.lib.edv_icp_scaled_workspace if scale else self.lib.edv_icp_workspace
        count = ICP_SCALED_TERMS if scale else ICP_TERMS
        if self.colour:
            count, cols = 2 * count, self.cols
            workspace = lambda h, w, step: self.lib.edv_icp_colour_workspace(h, w, step, cols)
        self.robust = None if robust is None else _check_robust(self.colour, **robust)
        if self.robust is not None:                                      # ``edv_icp_robust_sums``: one entry for all four, the same launches and reads
            self.name, cols, colour = "edv_icp_robust_sums", self.cols, int(self.colour)
            self.entry = self.lib.edv_icp_robust_sums
            workspace = lambda h, w, step: self.lib.edv_icp_robust_workspace(h, w, step, cols, colour)
        self.kinv = cams[frame if cams.shape[0] > 1 else 0, :9]
        self.max_dist2 = float(max_dist) * float(max_dist)
        self.model_cam = (C.c_double * 39)(*model_cam)
        self.size = views.size
        with torch.cuda.device(device):
            self.x = _on_device(depth, device)
            self.mask = None if mask is None else _staged(mask, device)
            self.sel = selection(self.x, spec, self.mask)
            self.depth, self.normals = _on_device(model.depth, device), _on_device(model.normals, device)
            if self.colour:
                self.frames, self.colors = _on_device(frames, device), _on_device(model.colors, device)
            self.live_normals = None
            if self.robust is not None and self.robust[0] is not None:   # the frame's own normals, once, with the gain of the spec
                self.live_normals = _frame_normals_device(self.lib, self.sel, _staged(cams, device), self.frame, 1, device)
            self.ws = torch.empty(max(int(workspace(h, w, int(spec.step))), 8), dtype=torch.uint8, device=device)
            self.sums_d = torch.empty(count, dtype=torch.float64, device=device)
            self.sums_h = torch.empty(count, dtype=torch.float64, pin_memory=True)

    def set_gain(self, gain) -> None:
        """The ``gain`` field of the selection struct rewritten with the float32 ``gain``: the struct travels by value with every launch."""
        self.sel.gain = float(np.float32(gain))

    def sums(self, live: np.ndarray) -> np.ndarray:
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if self.robust is not None:
                min_cos, huber, huber_colour = self.robust
                _lib.check(self.entry(C.byref(self.sel), self.frame, self.frames.data_ptr() if self.colour else None, (C.c_double * 21)(*live), self.model_cam,
                                      self.depth.data_ptr(), self.normals.data_ptr(), self.colors.data_ptr() if self.colour else None, self.size[0], self.size[1],
                                      self.max_dist2, self.cols, _lib.ptr(self.live_normals), -1.0 if min_cos is None else min_cos, huber, huber_colour,
                                      self.sums_d.data_ptr(), self.ws.data_ptr(), self.ws.numel(), C.c_void_p(stream.cuda_stream)), self.name)
            elif self.colour:
                _lib.check(self.entry(C.byref(self.sel), self.frame, self.frames.data_ptr(), (C.c_double * 21)(*live), self.model_cam, self.depth.data_ptr(),
                                      self.normals.data_ptr(), self.colors.data_ptr(), self.size[0], self.size[1], self.max_dist2, self.cols, self.sums_d.data_ptr(),
                                      self.ws.data_ptr(), self.ws.numel(), C.c_void_p(stream.cuda_stream)), self.name)
            else:
                _lib.check(self.entry(C.byref(self.sel), self.frame, (C.c_double * 21)(*live), self.model_cam, self.depth.data_ptr(), self.normals.data_ptr(),
                                      self.size[0], self.size[1], self.max_dist2, self.sums_d.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                      C.c_void_p(stream.cuda_stream)), self.name)
            self.sums_h.copy_(self.sums_d, non_blocking=True)
            stream.synchronize()
            return self.sums_h.numpy().copy()

    @staticmethod
    def placed(depth, frames):
        """The clip and its frames on the GPU, once: host arrays go to the current device, or to the depth tensor's; tensors stay as they are."""
        device = depth.device if isinstance(depth, torch.Tensor) and depth.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return _on_device(depth, device), None if frames is None else _on_device(frames, device)

    @staticmethod
    def pyramid(depth, spec, frame, levels, jump, frames):
        """The same on the GPU (``edv_depth_pyramid``, ``edv_rgb_pyramid``: a launch each, no host wait): the levels are tensors and stay there."""
        return ([d[None] for d in depth_pyramid(depth, spec, levels, jump, frame, output="device")],
                None if frames is None else [c[None] for c in rgb_pyramid(frames, levels, frame, output="device")])


def _estimate(ctx, spec: Cloud, frame: int) -> np.ndarray:
    return _live_cam(ctx.kinv, _pose4(spec.pose[frame if spec.pose.shape[0] > 1 else 0]))


def _check_scale(scale) -> bool:
    if not isinstance(scale, (bool, np.bool_)):
        raise ValueError(f"scale must be True or False, got {scale!r}")
    return bool(scale)


def icp_sums(depth, spec: Cloud, model: Raycast, views: Views, max_dist: float, frame: int = 0, scale: bool = False) -> np.ndarray:
    """float64 [29], or [37] with ``scale`` (the seventh column, for the scale ``spec.gain`` holds): the sums of one point-to-plane step (module docstring, "tracking") between frame ``frame`` of ``depth`` (float32 [n, h, w], a
    numpy array or a tensor on the GPU, as for ``Tsdf.integrate``), lifted through ``spec`` whose pose is the estimate, and ``model``, a one-view
    ``Raycast`` with normals (arrays or tensors) cast from ``views``.  On the GPU, on the caller's current stream; the host waits for the result."""
    ctx = _IcpDevice(depth, spec, model, views, max_dist, frame, scale=_check_scale(scale))
    return ctx.sums(_estimate(ctx, spec, frame))


def icp_sums_host(depth, spec: Cloud, model: Raycast, views: Views, max_dist: float, frame: int = 0, scale: bool = False) -> np.ndarray:
    """``icp_sums`` in numpy, the same operations in the same order: the two agree bit for bit."""
    ctx = _IcpHost(depth, spec, model, views, max_dist, frame, scale=_check_scale(scale))
    return ctx.sums(_estimate(ctx, spec, frame))


def _check_frames(frames):
    if frames is None:
        raise ValueError("the colour sums take the clip's frames, uint8 [n, h, w, 3]")
    return frames


def icp_colour_sums(depth, frames, spec: Cloud, model: Raycast, views: Views, max_dist: float, frame: int = 0, scale: bool = False) -> np.ndarray:
    """float64 [2, 29], or [2, 37] with ``scale``: row 0 is ``icp_sums`` of the same arguments, bit for bit, and row 1 the sums of the colour term
    (module docstring, "colour") over the same pairs: ``frames`` (uint8 [n, h, w, 3], an array or a tensor on the GPU) is the clip's RGB and
    ``model`` must carry ``colors``.  One tile launch forms both rows.  On the GPU, on the caller's current stream; the host waits for the result."""
    ctx = _IcpDevice(depth, spec, model, views, max_dist, frame, scale=_check_scale(scale), frames=_check_frames(frames))
    return ctx.sums(_estimate(ctx, spec, frame)).reshape(2, -1)


def icp_colour_sums_host(depth, frames, spec: Cloud, model: Raycast, views: Views, max_dist: float, frame: int = 0, scale: bool = False) -> np.ndarray:
    """``icp_colour_sums`` in numpy, the same operations in the same order: the two agree bit for bit."""
    ctx = _IcpHost(depth, spec, model, views, max_dist, frame, scale=_check_scale(scale), frames=_check_frames(frames))
    return ctx.sums(_estimate(ctx, spec, frame)).reshape(2, -1)


def icp_robust_sums(depth, spec: Cloud, model: Raycast, views: Views, max_dist: float, frame: int = 0, scale: bool = False, frames=None, min_cos: float = None,
                    huber: float = None, huber_colour: float = None) -> np.ndarray:
    """``icp_sums`` (float64 [29] or [37]) or, with ``frames`` and a model that carries ``colors``, ``icp_colour_sums`` ([2, 29] or [2, 37]) under the
    robust rule (module docstring, "robust"; ``edv_icp_robust_sums``).  ``min_cos``: the frame's own normals are formed (``frame_normals`` of that
    frame, with the gain of ``spec``) and a pair is kept only where they agree with the model's to that cosine; None: no test.  ``huber`` and
    ``huber_colour``: the Huber thresholds of the two residuals, positive; None or inf: no weight.  With all three off the sums have the bits of
    ``icp_sums`` or ``icp_colour_sums``.  On the GPU, on the caller's current stream; the host waits for the result."""
    ctx = _IcpDevice(depth, spec, model, views, max_dist, frame, scale=_check_scale(scale), frames=frames, robust=dict(min_cos=min_cos, huber=huber, huber_colour=huber_colour))
    sums = ctx.sums(_estimate(ctx, spec, frame))
    return sums if frames is None else sums.reshape(2, -1)


def icp_robust_sums_host(depth, spec: Cloud, model: Raycast, views: Views, max_dist: float, frame: int = 0, scale: bool = False, frames=None, min_cos: float = None,
                         huber: float = None, huber_colour: float = None) -> np.ndarray:
    """``icp_robust_sums`` in numpy, the same operations in the same order: the two agree bit for bit."""
    ctx = _IcpHost(depth, spec, model, views, max_dist, frame, scale=_check_scale(scale), frames=frames, robust=dict(min_cos=min_cos, huber=huber, huber_colour=huber_colour))
    sums = ctx.sums(_estimate(ctx, spec, frame))
    return sums if frames is None else sums.reshape(2, -1)


def _with_colour(sums: np.ndarray, weight: float) -> np.ndarray:
    """The T sums ``icp_solve`` takes from the 2 T of the colour path: A = A_g + weight^2 * A_c and b = b_g + weight^2 * b_c in float64; the last
    two entries, e e and the count, stay the geometric block's, and so do ``pairs``, ``rms`` and ``min_pairs``."""
    geometric, colour = sums.reshape(2, -1)
    out = geometric.copy()
    out[:-2] = geometric[:-2] + (weight * weight) * colour[:-2]
    return out


def icp_solve(sums, min_pairs):
    """The twist xi [6] (rotation vector, then translation) of the normal equations in the 29 ``sums``, or x [7] (the twist, then the scale's
    delta) of the 37, or None when the frame is lost: fewer than ``min_pairs`` pairs, a singular system, or a solution that is not finite."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.shape not in ((ICP_TERMS,), (ICP_SCALED_TERMS,)):
        raise ValueError(f"expected {ICP_TERMS} or {ICP_SCALED_TERMS} sums, got shape {tuple(sums.shape)}")
    m = _ICP_COLS[sums.shape[0]]
    tri = m * (m + 1) // 2
    if not sums[-1] >= min_pairs:
        return None
    A = np.zeros((m, m))
    A[np.triu_indices(m)] = sums[:tri]
    A = A + np.triu(A, 1).T
    try:
        xi = np.linalg.solve(A, sums[tri:tri + m])
    except np.linalg.LinAlgError:
        return None
    return xi if np.isfinite(xi).all() else None


def apply_twist(T, xi) -> np.ndarray:
    """T_world_camera [4, 4] moved by xi: R <- Rodrigues(xi[:3]) @ R about the camera centre, t <- t + xi[3:]."""
    T, xi = np.array(T, dtype=np.float64), np.asarray(xi, dtype=np.float64)
    theta = math.sqrt(float(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]))
    if theta > 0.0:
        a = xi[:3] / theta
        A = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        T[:3, :3] = (np.eye(3) + math.sin(theta) * A + (1.0 - math.cos(theta)) * (A @ A)) @ T[:3, :3]
    T[:3, 3] = T[:3, 3] + xi[3:]
    return T


def _pyramid_plan(track, spec: Cloud, h: int, w: int) -> list:
    """[(level, steps)] of the levels that are run, the coarsest first (module docstring, "pyramid"); without a pyramid [(0, iterations)]."""
    if track.pyramid is None:
        return [(0, track.iterations)]
    _check_level0(spec)
    if len(track.pyramid) > 1:
        _pyramid_sizes(h, w, len(track.pyramid) - 1)                     # every level holds a pixel, also one that is not run
    return [(level, steps) for level, steps in reversed(list(enumerate(track.pyramid))) if steps > 0]


def _track(tsdf, context, depth, spec, track, frame, frames=None):
    """``Tsdf.track`` and ``TsdfHost.track``: everything but the sums is this host code."""
    if not isinstance(track, Track):
        raise ValueError(f"track must be a fusion.Track, got {type(track).__name__}")
    n, h, w = _check_clip(depth, spec, None)
    if track.colour is None:
        frames = None                                                    # geometry alone: the frames are not looked at
    elif not tsdf.coloured or frames is None:
        raise ValueError("Track(colour=...) compares colours: it takes a coloured volume and the clip's frames")
    if isinstance(frame, bool) or not isinstance(frame, (int, np.integer)) or not 0 <= frame < n:
        raise ValueError(f"frame must be an integer in 0 .. {n - 1}, got {frame!r}")
    guess = _pose4(spec.pose[frame if spec.pose.shape[0] > 1 else 0])
    K = spec.K[frame if spec.K.shape[0] > 1 else 0]
    plan = _pyramid_plan(track, spec, h, w)                              # (level, steps), the coarsest level first; one resolution: [(0, iterations)]
    coarse = coarse_rgb = None
    if plan[0][0]:                                                       # the clip placed once for the pyramids and level 0; the levels once a frame, with the gain of the guess
        depth, frames = context.placed(depth, frames)
        coarse, coarse_rgb = context.pyramid(depth, spec, frame, plan[0][0], track.jump, frames)
    max_dist = tsdf.volume.trunc if track.max_dist is None else track.max_dist
    T, pairs, rms, sigma = guess.copy(), 0, float("nan"), 1.0
    lost = (guess, 1.0) if track.scale else (guess,)
    for level, steps in plan:
        if level == 0:
            clip, one, at, rgb, Kl = depth, spec, frame, frames, K
        else:                                                            # the stored level is an ordinary clip; the gain was kept out of it
            clip, at, rgb = coarse[level - 1], 0, None if frames is None else coarse_rgb[level - 1]
            Kl = K * np.array([[0.5 ** level], [0.5 ** level], [1.0]])  # exact: a power of two
            one = Cloud(K=Kl, pose=T, source="depth", gain=spec.gain, near=spec.near, far=spec.far)
        views = track.views(Kl, T, tuple(int(v) for v in clip.shape[1:3]))   # the model: cast from the current estimate, the guess for the first level
        model = tsdf.raycast(views, min_weight=track.min_weight, normals=True, output=context.output)
        ctx = context(clip, one, model, views, max_dist, at, scale=track.scale, frames=rgb, robust=track.robust() or None)   # the live normals: once a level, here
        for _ in range(steps):
            if track.scale:
                ctx.set_gain(np.float32(float(spec.gain) * sigma))
            sums = ctx.sums(_live_cam(ctx.kinv, T))
            if frames is not None:
                sums = _with_colour(sums, track.colour)
            pairs = int(sums[-1])
            rms = math.sqrt(sums[-2] / sums[-1]) if sums[-1] > 0.0 else float("nan")
            xi = icp_solve(sums, track.min_pairs)
            if xi is None:
                return lost[0], pairs, rms, True, *lost[1:]
            T = apply_twist(T, xi[:6])
            if track.scale:
                sigma = sigma * (1.0 + float(xi[6]))
                if not (math.isfinite(sigma) and sigma > 0.0 and 1.0 / (1.0 + track.max_scale_step) <= sigma <= 1.0 + track.max_scale_step):
                    return lost[0], pairs, rms, True, *lost[1:]
    U, _, Vt = np.linalg.svd(T[:3, :3])
    T[:3, :3] = U @ Vt
    return (T, pairs, rms, False, sigma) if track.scale else (T, pairs, rms, False)


def _track_clip(tsdf, depth, spec, track, frames):
    """``Tsdf.track_clip`` and ``TsdfHost.track_clip``."""
    if not isinstance(track, Track):
        raise ValueError(f"track must be a fusion.Track, got {type(track).__name__}")
    n, h, w, _, mask = _check_integrate(depth, spec, frames, tsdf.coloured)
    if track.colour is not None and not tsdf.coloured:
        raise ValueError("Track(colour=...) compares colours: it takes a coloured volume and the clip's frames")
    if spec.pose.shape[0] != 1:
        raise ValueError(f"tracking starts from one pose, the first camera's; the Cloud holds {spec.pose.shape[0]}")
    _pyramid_plan(track, spec, h, w)                                     # a pyramid the clip cannot have is refused before frame 0 is integrated
    out = Tracked(np.zeros((n, 4, 4)), np.zeros(n, np.int64), np.zeros(n), np.zeros(n, bool), np.ones(n) if track.scale else None)
    T, sigma = _pose4(spec.pose[0]), 1.0
    for i in range(n):
        one = dataclasses.replace(spec, K=spec.K[i if spec.K.shape[0] > 1 else 0], pose=T, mask=mask[i] if mask is not None and mask.ndim == 3 else mask)
        if track.scale:
            one = dataclasses.replace(one, gain=float(spec.gain) * sigma)     # the previous frame's scale: the guess
        if i:
            found, out.pairs[i], out.rms[i], out.lost[i], *factor = tsdf.track(depth[i:i + 1], one, track, frames=None if frames is None else frames[i:i + 1])
            if not out.lost[i]:
                T = found
                one = dataclasses.replace(one, pose=T)
                if track.scale:
                    sigma = sigma * factor[0]
                    one = dataclasses.replace(one, gain=float(spec.gain) * sigma)
        out.poses[i] = T
        if track.scale:
            out.scales[i] = sigma
        if not out.lost[i]:
            tsdf.integrate(depth[i:i + 1], one, None if frames is None else frames[i:i + 1])
    return out


class TsdfHost:
    """The numpy mirror of the kernels (module docstring): vectorised over the voxels, a loop over the frames."""

    def __init__(self, volume: Volume, coloured: bool = True):
        if not isinstance(volume, Volume):
            raise ValueError(f"volume must be a fusion.Volume, got {type(volume).__name__}")
        self.volume, self.coloured = volume, bool(coloured)
        self.reset()

    def reset(self) -> None:
        nx, ny, nz = self.volume.dims
        self.tsdf = np.ones((nz, ny, nx), np.float32)
        self.weight = np.zeros((nz, ny, nx), np.float32)
        self.color = np.zeros((nz, ny, nx, 3), np.float32) if self.coloured else None

    def arrays(self):
        """(tsdf, weight, color or None): copies."""
        return self.tsdf.copy(), self.weight.copy(), None if self.color is None else self.color.copy()

    def _index(self):
        nx, ny, nz = self.volume.dims
        a = np.arange(self.volume.voxels, dtype=np.int64)
        return a % nx, (a // nx) % ny, a // (nx * ny)

    def _gradients(self):
        """float32 [voxels, 3]: g_k = tsdf[i_k -> min(i_k + 1, n_k - 1)] - tsdf[i_k -> max(i_k - 1, 0)] of every voxel."""
        nx, ny, nz = self.volume.dims
        return np.stack([np.take(self.tsdf, np.minimum(np.arange(n) + 1, n - 1), axis=ax) - np.take(self.tsdf, np.maximum(np.arange(n) - 1, 0), axis=ax)
                         for ax, n in ((2, nx), (1, ny), (0, nz))], axis=-1).reshape(-1, 3)

    def integrate(self, depth, spec: Cloud, frames=None) -> None:
        depth = np.asarray(depth)
        n, h, w, cams, mask = _check_integrate(depth, spec, frames, self.coloured)
        vol = self.volume
        origin, voxel, trunc = np.float64(vol.origin), np.float64(vol.voxel), np.float64(vol.trunc)
        cap, one = np.float32(vol.max_weight), np.float32(1.0)
        lo, span, gain, near, far = spec.scalars()
        cx, cy, cz = (origin[k] + (i.astype(np.float64) + 0.5) * voxel for k, i in enumerate(self._index()))
        t, wt = self.tsdf.reshape(-1), self.weight.reshape(-1)           # views: updated in place
        col = None if self.color is None else self.color.reshape(-1, 3)
        rgb = None if frames is None else np.asarray(frames)
        for f in range(n):
            cam = cams[f if cams.shape[0] > 1 else 0]
            W, K = cam[:12].reshape(3, 4), cam[12:].reshape(2, 3)
            with np.errstate(all="ignore"):
                q = [((W[i, 0] * cx + W[i, 1] * cy) + W[i, 2] * cz) + W[i, 3] for i in range(3)]
                ok = q[2] > 0.0
                u = ((K[0, 0] * q[0] + K[0, 1] * q[1]) + K[0, 2] * q[2]) / q[2]
                v = ((K[1, 0] * q[0] + K[1, 1] * q[1]) + K[1, 2] * q[2]) / q[2]
                ok &= (u >= 0.0) & (u < float(w)) & (v >= 0.0) & (v < float(h))
                px, py = np.where(ok, u, 0.0).astype(np.int64), np.where(ok, v, 0.0).astype(np.int64)
                x = depth[f][py, px]
                if spec.source == "depth":
                    z = x * gain
                else:
                    scaled = lo + span * x
                    z = one / scaled
                    z = z * gain
                ok &= (z > near) & (z < far)
                if mask is not None:
                    ok &= (mask[f] if mask.ndim == 3 else mask)[py, px] != 0
                sdf = z.astype(np.float64) - q[2]
                ok &= ~(sdf < -trunc)
                ratio = sdf / trunc
                d = np.where(ratio < 1.0, ratio, 1.0).astype(np.float32)
                wn = wt + one
                t[:] = np.where(ok, (t * wt + d) / wn, t)
                if col is not None:
                    c = rgb[f][py, px].astype(np.float32)
                    col[:] = np.where(ok[:, None], (col * wt[:, None] + c) / wn[:, None], col)
                wt[:] = np.where(ok, np.where(wn < cap, wn, cap), wt)

    def surface(self, min_weight: float = 1.0, output: str = "host") -> PointCloud:
        mw = _check_surface(min_weight, output)
        if output != "host":
            raise ValueError("the host mirror has no device output")
        vol = self.volume
        nx, ny, nz = vol.dims
        origin, voxel = np.float64(vol.origin), np.float64(vol.voxel)
        idx = self._index()
        t, wt = self.tsdf.reshape(-1), self.weight.reshape(-1)
        N = vol.voxels
        cross, tb = np.zeros((N, 3), bool), np.zeros((N, 3), np.float32)
        hop = (1, nx, nx * ny)
        for k in range(3):
            a = np.nonzero(idx[k] + 1 < vol.dims[k])[0]
            b = a + hop[k]
            cross[a, k] = (wt[a] >= mw) & (wt[b] >= mw) & ((t[a] < 0) != (t[b] < 0))
            tb[a, k] = t[b]
        a, k = np.nonzero(cross)                                     # row-major: voxel-major, axis-minor
        with np.errstate(all="ignore"):
            frac = t[a] / (t[a] - tb[a, k])
            points = np.empty((a.shape[0], 3), np.float32)
            for j in range(3):
                ctr = idx[j][a].astype(np.float64) + 0.5
                points[:, j] = (origin[j] + np.where(k == j, ctr + frac.astype(np.float64), ctr) * voxel).astype(np.float32)
            colors = None
            if self.color is not None:
                col = self.color.reshape(-1, 3)
                ca, cb = col[a], col[a + np.asarray(hop, np.int64)[k]]
                c = ca + frac[:, None] * (cb - ca)
                colors = np.minimum(np.float32(255.0), np.maximum(np.float32(0.0), np.floor(c + np.float32(0.5)))).astype(np.uint8)
        return PointCloud(points, colors, np.array([0, a.shape[0]], np.int64))

    def mesh(self, min_weight: float = 1.0, normals: bool = True, output: str = "host") -> Mesh:
        """The triangle mesh of the volume (module docstring, "mesh"), vectorised over the voxels."""
        mw = _check_mesh(min_weight, normals, output)
        if output != "host":
            raise ValueError("the host mirror has no device output")
        vol = self.volume
        nx, ny, nz = vol.dims
        origin, voxel = np.float64(vol.origin), np.float64(vol.voxel)
        ix, iy, iz = idx = self._index()
        t, wt = self.tsdf.reshape(-1), self.weight.reshape(-1)
        N = vol.voxels
        hop = np.array([dx + nx * (dy + ny * dz) for dx, dy, dz in OFFSETS], np.int64)
        observed, inside = wt >= mw, t < 0
        valid = np.zeros(N, bool)
        cells = np.nonzero((ix + 1 < nx) & (iy + 1 < ny) & (iz + 1 < nz))[0]
        valid[cells] = np.all([observed[cells + hop[c]] for c in range(8)], axis=0)
        carries = np.zeros((N, 7), bool)                             # [a, d - 1]: edge (a, d) carries a vertex
        for d in range(1, 8):
            dx, dy, dz = OFFSETS[d]
            a = np.nonzero((ix + dx < nx) & (iy + dy < ny) & (iz + dz < nz))[0]
            used = np.zeros(a.shape[0], bool)
            for s in range(8):
                if s & d == 0:
                    sx, sy, sz = OFFSETS[s]
                    there = (ix[a] >= sx) & (iy[a] >= sy) & (iz[a] >= sz)
                    used[there] |= valid[a[there] - hop[s]]
            carries[a, d - 1] = observed[a] & observed[a + hop[d]] & (inside[a] != inside[a + hop[d]]) & used
        rank = np.cumsum(carries, axis=1) - carries                   # vertices of the same voxel with a smaller d
        owned = carries.sum(axis=1)
        first = np.cumsum(owned) - owned                              # the index of a voxel's first vertex
        a, k = np.nonzero(carries)                                    # row-major: voxel-major, d-minor
        d = k + 1
        b = a + hop[d]
        with np.errstate(all="ignore"):
            frac = t[a] / (t[a] - t[b])
            vertices = np.empty((a.shape[0], 3), np.float32)
            for j in range(3):
                ctr = idx[j][a].astype(np.float64) + 0.5
                vertices[:, j] = (origin[j] + np.where((d >> j) & 1 == 1, ctr + frac.astype(np.float64), ctr) * voxel).astype(np.float32)
            unit = None
            if normals:
                g = self._gradients()
                n = g[a] + frac[:, None] * (g[b] - g[a])
                length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
                unit = np.where((length > 0)[:, None], n / length[:, None], np.float32(0.0)).astype(np.float32)
            colors = None
            if self.color is not None:
                col = self.color.reshape(-1, 3)
                c = col[a] + frac[:, None] * (col[b] - col[a])
                colors = np.minimum(np.float32(255.0), np.maximum(np.float32(0.0), np.floor(c + np.float32(0.5)))).astype(np.uint8)
        cells = np.nonzero(valid)[0]
        pattern = np.stack([inside[cells + hop[c]] for c in range(8)], axis=1)
        case = np.stack([sum(pattern[:, c].astype(np.int64) << i for i, c in enumerate(corners)) for corners in TETRAHEDRA], axis=1)
        edges = MESH_TABLE[np.arange(6)[None, :], case].astype(np.int64)      # [cells, 6, 2, 3, 2]
        cell, ti, tri = np.nonzero(edges[..., 0, 0] >= 0)                     # row-major: cell-major, then tetrahedron, then triangle
        u, dd = edges[cell, ti, tri, :, 0], edges[cell, ti, tri, :, 1]
        w = cells[cell][:, None] + hop[u]
        triangles = (first[w] + rank[w, dd - 1]).astype(np.int32).reshape(-1, 3)
        return Mesh(vertices, unit, colors, triangles)


    def raycast(self, views: Views, min_weight: float = 1.0, normals: bool = True, output: str = "host") -> Raycast:
        """The volume as ``views`` see it (module docstring, "views"), vectorised over the pixels of a view: a loop over the steps on the
        rays still marching."""
        mw = _check_raycast(views, min_weight, normals, output)
        if output != "host":
            raise ValueError("the host mirror has no device output")
        vol = self.volume
        dims = nx, ny, nz = vol.dims
        step, steps = views.march(vol.voxel)
        cams, near, (h, w), m = views.cams(), views.near, views.size, views.count
        origin, inv = np.float64(vol.origin), 1.0 / vol.voxel
        depth = np.zeros((m, h * w), np.float32)
        unit = np.zeros((m, h * w, 3), np.float32) if normals else None
        colors = np.zeros((m, h * w, 3), np.uint8) if self.color is not None else None
        shaped = Raycast(depth.reshape(m, h, w), None if unit is None else unit.reshape(m, h, w, 3), None if colors is None else colors.reshape(m, h, w, 3))
        if min(dims) < 2:                                                # no cell: every pixel is a miss
            return shaped
        t, wt = self.tsdf.reshape(-1), self.weight.reshape(-1)
        hop = np.array([dx + nx * (dy + ny * dz) for dx, dy, dz in OFFSETS], np.int64)
        u = np.broadcast_to((np.arange(w, dtype=np.float64) + 0.5)[None, :], (h, w)).reshape(-1)
        v = np.broadcast_to((np.arange(h, dtype=np.float64) + 0.5)[:, None], (h, w)).reshape(-1)
        top = np.array(dims, np.float64)[:, None] - 1.0
        grads = self._gradients() if normals else None
        for f in range(m):
            kinv, rot, pos = cams[f, :9].reshape(3, 3), cams[f, 9:18].reshape(3, 3), cams[f, 18:]
            with np.errstate(all="ignore"):
                l = [(kinv[i, 0] * u + kinv[i, 1] * v) + kinv[i, 2] for i in range(3)]
                r = [(rot[i, 0] * l[0] + rot[i, 1] * l[1]) + rot[i, 2] * l[2] for i in range(3)]
                o = np.stack([np.full(h * w, (pos[i] - origin[i]) * inv - 0.5) for i in range(3)])
                d = np.stack([r[i] * inv for i in range(3)])
                alive = np.arange(h * w)                                 # the rays still marching
                have, sp = np.zeros(h * w, bool), np.zeros(h * w, np.float32)
                hits, hit_k, hit_t = [], [], []
                for k in range(steps):
                    if alive.size == 0:
                        break
                    z = near + float(k) * step
                    g = o[:, alive] + d[:, alive] * z
                    ok = ((g >= 0.0) & (g <= top)).all(axis=0)           # inside; NaN fails
                    c, fr = _cell(g[:, ok], dims)
                    a = c[0] + nx * (c[1] + ny * c[2])
                    valid = (wt[a[None, :] + hop[:, None]] >= mw).all(axis=0)
                    ok[ok] = valid
                    s = _trilinear(t[a[None, valid] + hop[:, None]], fr[:, valid])
                    rays = alive[ok]
                    inside = s < 0                                       # 0 and -0 count as outside
                    hit = inside & have[rays]
                    hits.append(rays[hit])
                    hit_k.append(np.full(int(hit.sum()), k - 1, np.int64))
                    hit_t.append(sp[rays[hit]] / (sp[rays[hit]] - s[hit]))
                    have[alive] = False                                  # a sample that is not valid forgets the previous one
                    have[rays[~inside]], sp[rays[~inside]] = True, s[~inside]
                    done = np.zeros(alive.size, bool)
                    done[ok] = inside                                    # a hit, or a miss that entered the surface unseen
                    alive = alive[~done]
                rays, frac = np.concatenate(hits), np.concatenate(hit_t)
                zs = (near + np.concatenate(hit_k).astype(np.float64) * step) + frac.astype(np.float64) * step
                depth[f, rays] = zs.astype(np.float32)
                c, fr = _cell(o[:, rays] + d[:, rays] * zs, dims)        # the clamp keeps the cell in the grid whatever the rounding
                corners = (c[0] + nx * (c[1] + ny * c[2]))[None, :] + hop[:, None]
                if normals:
                    n = _trilinear(grads[corners], fr)
                    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
                    unit[f, rays] = np.where((length > 0)[:, None], n / length[:, None], np.float32(0.0)).astype(np.float32)
                if colors is not None:
                    col = _trilinear(self.color.reshape(-1, 3)[corners], fr)
                    colors[f, rays] = np.minimum(np.float32(255.0), np.maximum(np.float32(0.0), np.floor(col + np.float32(0.5)))).astype(np.uint8)
        return shaped

    def track(self, depth, spec: Cloud, track: Track, frame: int = 0, frames=None):
        """The mirror of ``Tsdf.track``: the same host code around ``icp_sums_host``; a 5-tuple that ends with the scale factor with ``track.scale``."""
        return _track(self, _IcpHost, np.asarray(depth), spec, track, frame, None if frames is None else np.asarray(frames))

    def track_clip(self, depth, spec: Cloud, track: Track, frames=None) -> Tracked:
        """The mirror of ``Tsdf.track_clip``."""
        return _track_clip(self, np.asarray(depth), spec, track, None if frames is None else np.asarray(frames))


class Tsdf:
    """A TSDF volume on the GPU.  ``integrate`` folds clips into it, ``surface`` and ``mesh`` read its zero crossings, ``raycast`` views it from
    cameras; all run on the caller's current stream.  ``arrays`` and the tensors ``tsdf``, ``weight`` and ``color`` show the state."""

    def __init__(self, volume: Volume, coloured: bool = True, device="cuda"):
        if not isinstance(volume, Volume):
            raise ValueError(f"volume must be a fusion.Volume, got {type(volume).__name__}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"a Tsdf lives on the GPU (fusion.TsdfHost is the numpy mirror), got device {device!r}")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self.volume, self.coloured = volume, bool(coloured)
        self._lib = _lib.load()
        nx, ny, nz = volume.dims
        with torch.cuda.device(self.device):
            self.tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
            self.weight = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
            self.color = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=self.device) if self.coloured else None
        self.reset()

    def reset(self) -> None:
        with torch.cuda.device(self.device):
            self.tsdf.fill_(1.0)
            self.weight.zero_()
            if self.color is not None:
                self.color.zero_()

    def arrays(self):
        """(tsdf, weight, color or None) as numpy arrays: host copies."""
        with torch.cuda.device(self.device):
            return self.tsdf.cpu().numpy(), self.weight.cpu().numpy(), None if self.color is None else self.color.cpu().numpy()

    def struct(self) -> _lib.TsdfVolume:
        """The ``edv_tsdf_volume`` of this volume."""
        v = self.volume
        return _lib.TsdfVolume(self.tsdf.data_ptr(), self.weight.data_ptr(), _lib.ptr(self.color), v.dims[0], v.dims[1], v.dims[2],
                               (C.c_double * 3)(*v.origin), v.voxel, v.trunc, float(np.float32(v.max_weight)))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def integrate(self, depth, spec: Cloud, frames=None) -> None:
        """``depth``: float32 [n, h, w], a numpy array or a tensor on this volume's GPU, which is used in place with no copy.  ``frames``: uint8
        [n, h, w, 3] (array or tensor), required by a coloured volume.  One launch on the caller's current stream, ordered on that stream; the
        host does not wait for it."""
        if isinstance(depth, torch.Tensor):
            if not depth.is_cuda or depth.device != self.device:
                raise ValueError(f"a depth tensor must live on the volume's GPU {self.device} (pass host data as a numpy array)")
        else:
            depth = np.asarray(depth)
        n, h, w, cams, mask = _check_integrate(depth, spec, frames, self.coloured)
        with torch.cuda.device(self.device):
            x = _on_device(depth, self.device)
            rgb = None if frames is None else _on_device(frames, self.device)
            mask_d = None if mask is None else _staged(mask, self.device)
            cams_d = _staged(cams, self.device)
            sel = selection(x, spec, mask_d)
            vol = self.struct()
            _lib.check(self._lib.edv_tsdf_integrate(C.byref(vol), C.byref(sel), cams_d.data_ptr(), 18 if cams.shape[0] > 1 else 0, _lib.ptr(rgb),
                                                    self._stream()), "edv_tsdf_integrate")

    def surface(self, min_weight: float = 1.0, output: str = "host") -> PointCloud:
        """The zero crossings between voxels of weight >= ``min_weight``: the count, one read of the total (the one host synchronisation), an
        exact allocation, the extract.  Returns a ``cloud.PointCloud`` with ``offsets = [0, total]``: numpy arrays, or with ``output="device"``
        tensors on the GPU, ordered on the caller's stream.  ``colors`` is None for an uncoloured volume."""
        mw = float(_check_surface(min_weight, output))
        lib, dev, v = self._lib, self.device, self.volume
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            st = self._stream()
            vol = self.struct()
            ws = torch.empty(int(lib.edv_tsdf_workspace(*v.dims)), dtype=torch.uint8, device=dev)
            total_d = torch.empty(1, dtype=torch.int64, device=dev)
            _lib.check(lib.edv_tsdf_count(C.byref(vol), mw, total_d.data_ptr(), ws.data_ptr(), ws.numel(), st), "edv_tsdf_count")
            total_h = torch.empty(1, dtype=torch.int64, pin_memory=True)
            total_h.copy_(total_d, non_blocking=True)
            stream.synchronize()
            total = int(total_h[0])
            offsets = np.array([0, total], np.int64)
            points = torch.empty((total, 3), dtype=torch.float32, device=dev)
            colors = torch.empty((total, 3), dtype=torch.uint8, device=dev) if self.coloured else None
            if total:  # an empty surface launches nothing
                _lib.check(lib.edv_tsdf_extract(C.byref(vol), mw, ws.data_ptr(), ws.numel(), points.data_ptr(), _lib.ptr(colors), total, st), "edv_tsdf_extract")
            if output == "device":
                return PointCloud(points, colors, offsets)
            host_p = torch.empty((total, 3), dtype=torch.float32, pin_memory=True)
            host_p.copy_(points, non_blocking=True)
            host_c = None
            if colors is not None:
                host_c = torch.empty((total, 3), dtype=torch.uint8, pin_memory=True)
                host_c.copy_(colors, non_blocking=True)
            stream.synchronize()
            return PointCloud(host_p.numpy(), None if host_c is None else host_c.numpy(), offsets)

    def mesh(self, min_weight: float = 1.0, normals: bool = True, output: str = "host") -> Mesh:
        """The triangle mesh of the volume between voxels of weight >= ``min_weight`` (module docstring, "mesh"): the count, one read of the two
        totals (the one host synchronisation), exact allocations, the extract.  Returns a ``Mesh`` of numpy arrays, or with ``output="device"``
        of tensors on the GPU, ordered on the caller's stream.  ``normals=False`` leaves them out; ``colors`` is None for an uncoloured volume."""
        mw = float(_check_mesh(min_weight, normals, output))
        lib, dev, v = self._lib, self.device, self.volume
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            st = self._stream()
            vol = self.struct()
            ws = torch.empty(int(lib.edv_tsdf_mesh_workspace(*v.dims)), dtype=torch.uint8, device=dev)
            totals_d = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(lib.edv_tsdf_mesh_count(C.byref(vol), mw, totals_d.data_ptr(), ws.data_ptr(), ws.numel(), st), "edv_tsdf_mesh_count")
            totals_h = torch.empty(2, dtype=torch.int64, pin_memory=True)
            totals_h.copy_(totals_d, non_blocking=True)
            stream.synchronize()
            nv, nt = int(totals_h[0]), int(totals_h[1])
            if nv >= 2 ** 31:
                raise ValueError(f"a mesh holds fewer than 2^31 vertices (its indices are int32), this one has {nv}")
            shapes = [((nv, 3), torch.float32), ((nv, 3), torch.float32) if normals else None, ((nv, 3), torch.uint8) if self.coloured else None,
                      ((nt, 3), torch.int32)]
            out = [None if s is None else torch.empty(s[0], dtype=s[1], device=dev) for s in shapes]
            if nv or nt:  # an empty mesh launches nothing
                _lib.check(lib.edv_tsdf_mesh_extract(C.byref(vol), mw, ws.data_ptr(), ws.numel(), out[0].data_ptr(), _lib.ptr(out[1]), _lib.ptr(out[2]), nv,
                                                     out[3].data_ptr(), nt, st), "edv_tsdf_mesh_extract")
            if output == "device":
                return Mesh(*out)
            host = [None if o is None else torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in out]
            for h, o in zip(host, out):
                if h is not None:
                    h.copy_(o, non_blocking=True)
            stream.synchronize()
            return Mesh(*(None if h is None else h.numpy() for h in host))


    def raycast(self, views: Views, min_weight: float = 1.0, normals: bool = True, output: str = "host") -> Raycast:
        """The volume as ``views`` see it (module docstring, "views"): a depth map, and unless ``normals=False`` a normal map, and for a coloured
        volume a colour image, per view.  One launch on the caller's current stream, the cameras staged through pinned memory.  Returns a
        ``Raycast`` of numpy arrays, or with ``output="device"`` of tensors on the GPU ordered on the caller's stream; the host waits only for
        the copy of a host result."""
        mw = float(_check_raycast(views, min_weight, normals, output))
        step, steps = views.march(self.volume.voxel)
        m, (h, w) = views.count, views.size
        dev = self.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            cams_d = _staged(views.cams(), dev)
            shapes = [((m, h, w), torch.float32), ((m, h, w, 3), torch.float32) if normals else None, ((m, h, w, 3), torch.uint8) if self.coloured else None]
            out = [None if s is None else torch.empty(s[0], dtype=s[1], device=dev) for s in shapes]
            vol = self.struct()
            _lib.check(self._lib.edv_tsdf_raycast(C.byref(vol), cams_d.data_ptr(), m, h, w, views.near, step, steps, mw, out[0].data_ptr(), _lib.ptr(out[1]),
                                                  _lib.ptr(out[2]), self._stream()), "edv_tsdf_raycast")
            if output == "device":
                return Raycast(*out)
            host = [None if o is None else torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in out]
            for hst, o in zip(host, out):
                if hst is not None:
                    hst.copy_(o, non_blocking=True)
            stream.synchronize()
            return Raycast(*(None if hst is None else hst.numpy() for hst in host))

    def _own(self, depth):
        if isinstance(depth, torch.Tensor) and (not depth.is_cuda or depth.device != self.device):
            raise ValueError(f"a depth tensor must live on the volume's GPU {self.device} (pass host data as a numpy array)")
        return depth if isinstance(depth, torch.Tensor) else np.asarray(depth)

    def track(self, depth, spec: Cloud, track: Track, frame: int = 0, frames=None):
        """The pose of frame ``frame`` of ``depth`` (as for ``integrate``) against this volume (module docstring, "tracking"): the volume ray-cast
        once from the guess, which is ``spec.pose`` with ``spec.K`` and the frame's size, then ``track.iterations`` steps of sums on the GPU, a
        6 x 6 solve on the host and the twist applied.  Returns (T_world_camera float64 [4, 4], pairs, rms, lost); a lost frame returns the
        guess.  With ``track.scale`` the system is 7 x 7 and the tuple ends with the scale factor found, a Python float relative to
        ``spec.gain``, 1.0 for a lost frame.  With ``track.colour`` the volume must be coloured and ``frames`` (uint8 [n, h, w, 3], as for
        ``integrate``) given: every pair also compares the frame's intensity with the model's (module docstring, "colour"); otherwise ``frames``
        is not looked at.  With ``track.pyramid`` the steps run coarse to fine (module docstring, "pyramid"): the frame's depth and colour levels
        are formed once (a launch each) and stay on the GPU, every level that is run ray-casts the volume at its own size from the current
        estimate, and ``iterations`` is not used.  On the caller's current stream; the host waits once per step."""
        with torch.cuda.device(self.device):
            return _track(self, _IcpDevice, self._own(depth), spec, track, frame, frames)

    def track_clip(self, depth, spec: Cloud, track: Track, frames=None) -> Tracked:
        """A clip whose first camera alone is known: ``spec`` holds one pose.  Frame 0 is integrated there; every later frame is tracked from the
        previous frame's pose (with ``track.scale`` also from its scale, and integrated with the scale found: ``Tracked.scales``) and integrated at
        the pose found; a lost frame keeps the previous pose and is not integrated.  ``depth`` and
        ``frames`` as for ``integrate``, placed on the GPU once.  With ``track.colour`` frame i is tracked with ``frames[i:i+1]`` too, which takes a
        coloured volume."""
        with torch.cuda.device(self.device):
            depth = _on_device(self._own(depth), self.device)
            return _track_clip(self, depth, spec, track, None if frames is None else _on_device(frames, self.device))


def _face_dtype():
    return np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _mesh_vertex_dtype(normals: bool, colours: bool):
    fields = [(n, "<f4") for n in "xyz"] + ([(n, "<f4") for n in ("nx", "ny", "nz")] if normals else []) + ([(n, "u1") for n in ("red", "green", "blue")] if colours else [])
    return np.dtype(fields)


def _mesh_header(nv, nf, normals, colours):
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {nv}", "property float x", "property float y", "property float z"]
    if normals:
        header += ["property float nx", "property float ny", "property float nz"]
    if colours:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    return header + [f"element face {nf}", "property list uchar int vertex_indices", "end_header"]


def write_mesh_ply(path, mesh: Mesh) -> None:
    """Binary little-endian ``.ply``: vertices ``x y z`` float, then ``nx ny nz`` float and ``red green blue`` uchar where the mesh has them, and
    faces as ``property list uchar int vertex_indices``.  Tensors on the GPU are copied to the host first."""
    parts = [None if p is None else (p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)) for p in (mesh.vertices, mesh.normals, mesh.colors, mesh.triangles)]
    vertices, normals, colors, triangles = parts
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    vertex = np.empty(vertices.shape[0], _mesh_vertex_dtype(normals is not None, colors is not None))
    columns = list(zip("xyz", vertices.T))
    if normals is not None:
        columns += list(zip(("nx", "ny", "nz"), np.asarray(normals, np.float32).reshape(-1, 3).T))
    if colors is not None:
        columns += list(zip(("red", "green", "blue"), np.asarray(colors, np.uint8).reshape(-1, 3).T))
    for name, column in columns:
        if column.shape[0] != vertex.shape[0]:
            raise ValueError(f"{name}: {column.shape[0]} values for {vertex.shape[0]} vertices")
        vertex[name] = column
    triangles = np.asarray(triangles, np.int32).reshape(-1, 3)
    face = np.empty(triangles.shape[0], _face_dtype())
    face["n"], face["v"] = 3, triangles
    with open(path, "wb") as fh:
        fh.write(("\n".join(_mesh_header(vertex.shape[0], face.shape[0], normals is not None, colors is not None)) + "\n").encode("ascii"))
        fh.write(vertex.tobytes())
        fh.write(face.tobytes())


def read_mesh_ply(path) -> Mesh:
    """A ``.ply`` as ``write_mesh_ply`` writes it -> ``Mesh`` of numpy arrays."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a .ply file")
    lines = data[:end].decode("ascii").split("\n")[:-1] + ["end_header"]
    try:
        nv, nf = int(lines[2].split()[2]), int(next(ln for ln in lines if ln.startswith("element face ")).split()[2])
    except (IndexError, ValueError, StopIteration):
        raise ValueError(f"{path}: expected a binary little-endian .ply with vertices, then faces") from None
    for normals, colours in itertools.product((False, True), repeat=2):
        if lines == _mesh_header(nv, nf, normals, colours):
            break
    else:
        raise ValueError(f"{path}: not a header write_mesh_ply writes")
    vdt, fdt = _mesh_vertex_dtype(normals, colours), _face_dtype()
    body = data[end + len(b"end_header\n"):]
    if len(body) != nv * vdt.itemsize + nf * fdt.itemsize:
        raise ValueError(f"{path}: {len(body)} bytes after the header, which says {nv} x {vdt.itemsize} + {nf} x {fdt.itemsize}")
    vertex, face = np.frombuffer(body, vdt, nv), np.frombuffer(body, fdt, nf, offset=nv * vdt.itemsize)
    if not (face["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")

    def columns(names, dtype):
        return np.stack([vertex[n] for n in names], axis=1).astype(dtype) if nv else np.empty((0, 3), dtype)

    return Mesh(columns("xyz", np.float32), columns(("nx", "ny", "nz"), np.float32) if normals else None,
                columns(("red", "green", "blue"), np.uint8) if colours else None, face["v"].astype(np.int32).reshape(-1, 3))
