/* softgrip.h -- C ABI of the MI355X-native batched soft-gripper simulator.
 *
 * This is the boundary the reference crosses through mujoco_py; every
 * entry point names the mujoco_py call it replaces in reference environment/manenv.py.
 * All functions return 0 on success or a negative sg_status; sg_last_error() gives the
 * message of the last failure on the calling thread.  Per-env numeric failure is DATA
 * (the `flags` output), not an error code.
 *
 * Memory: the library owns models and batch state (device memory).  Callers own every
 * output buffer and pass raw pointers (device pointers unless stated otherwise; with
 * PyTorch-ROCm: tensor.data_ptr()).  `stream` is a hipStream_t (NULL = default stream);
 * no function synchronises the host unless it says so.
 *
 * A batch is externally synchronised (one caller thread at a time); different batches,
 * e.g. one per GPU, are fully independent.  No CPU fallback exists: creating a batch on
 * a machine without a HIP device fails with SG_ERR_NO_DEVICE.
 */
#ifndef SOFTGRIP_H
#define SOFTGRIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sg_model sg_model;
typedef struct sg_batch sg_batch;

typedef enum sg_status {
  SG_OK = 0,
  SG_ERR_INVALID = -1,     /* bad argument */
  SG_ERR_MODEL = -2,       /* blob malformed or model outside the supported class */
  SG_ERR_NO_DEVICE = -3,   /* no HIP device / device index out of range */
  SG_ERR_HIP = -4,         /* a HIP runtime call failed */
  SG_ERR_NOMEM = -5
} sg_status;

/* per-env flag bits written by sg_step/sg_reset (any of 1|2|4|8|16|32 is what mujoco_py
 * would have turned into MujocoException, reference environment/manenv.py:50) */
enum {
  SG_FLAG_BADQPOS = 1, SG_FLAG_BADQVEL = 2, SG_FLAG_BADQACC = 4,
  SG_FLAG_CONTACTFULL = 8, SG_FLAG_CNSTRFULL = 16, SG_FLAG_UNSUPPORTED_PAIR = 32
};

const char* sg_last_error(void);
const char* sg_version(void);

/* ---- model: replaces mujoco_py.load_model_from_path (manenv.py:27,36).
 * sg_model_compile: MJCF file -> model: the native compiler of the MJCF subset the soft-gripper scenes use
 *   (csrc/sg_mjcf.cpp; <include>s resolved relative to the file's directory), then sg_model_create.  flags: SG_COMPILE_*.
 * sg_mjcf_compile: the same compiler, returning the blob of softgrip_model.h (malloc'd: release with sg_blob_free) -- e.g. to
 *   store a compiled scene.  The Python host has its own implementation of the same compiler (soft-grip_amd/mjcf.py);
 *   tests/test_mjcf.py holds the two against each other.
 * sg_model_create: validates a blob and derives the kernel plan.  Host pointers throughout. */
enum {
  SG_COMPILE_NO_NEIGHBORS = 1,            /* leave out the composite's neighbour equalities (models/<scene>_fix) */
  SG_COMPILE_IMPLICIT_TENDON_DAMPER = 2   /* opt_i[3] = 1: implicit volume-tendon damper */
};
int sg_model_compile(const char* xml_path, int flags, sg_model** out);
int sg_mjcf_compile(const char* xml_path, int flags, void** blob, size_t* nbytes);
void sg_blob_free(void* blob);
int sg_model_create(const void* blob, size_t nbytes, sg_model** out);
void sg_model_destroy(sg_model* m);
int sg_model_nq(const sg_model* m);           /* positions; == nv unless the model has a free joint (7 positions, 6 dofs) */
int sg_model_nv(const sg_model* m);           /* dofs: the width of qvel / qacc_warmstart */
int sg_model_njnt(const sg_model* m);         /* joints: what the ids of sg_set_stiffness count */
int sg_model_nu(const sg_model* m);           /* == na */
int sg_model_nsensordata(const sg_model* m);
int sg_model_ntendon(const sg_model* m);
int sg_model_nelem(const sg_model* m);

/* ---- batch of n_envs independent simulations: replaces mujoco_py.MjSim(model)
 * (manenv.py:28,37), one MjSim per env.  State starts as after mj_resetData. */
int sg_batch_create(const sg_model* m, int n_envs, int device, sg_batch** out);
void sg_batch_destroy(sg_batch* b);
int sg_batch_nenvs(const sg_batch* b);
int sg_batch_device(const sg_batch* b);

/* replaces `model.jnt_stiffness[i] = k` / `model.tendon_stiffness[i] = k`
 * (manenv.py:105-108): env e uses k[e] on the listed joint and tendon ids and the model's
 * own stiffness everywhere else.  k: device or host pointer to n_envs doubles
 * (k_on_host selects); ids: host pointers.  The id sets replace those of earlier calls.
 * SYNCHRONISES THE HOST with `stream` when k is a host pointer or when the id sets differ
 * from the previous call's (once per scene; the step path never calls it): with a device k
 * and unchanged id sets it enqueues one copy on `stream` and returns. */
int sg_set_stiffness(sg_batch* b, const double* k, int k_on_host, const int* jnt_ids, int nj, const int* ten_ids, int nt,
                     void* stream);

/* replaces `data.ctrl[i] = v` (manenv.py:95,100).  ctrl: HOST pointer to nu doubles when
 * broadcast != 0 (same control for every env), else device pointer to [n_envs][nu]. */
int sg_set_ctrl(sg_batch* b, const double* ctrl, int broadcast, void* stream);

/* replaces sim.reset(); sim.forward(); then `sim_start` x sim.step()  (manenv.py:57-61)
 * for the envs whose mask byte is non-zero (mask == NULL: all).  mask: device pointer to
 * n_envs bytes.  ctrl of the reset envs is zeroed (mj_resetData).  Outputs as sg_step. */
int sg_reset(sg_batch* b, const uint8_t* mask, int sim_start, double* sens_out, int32_t* flags_out, int32_t* touch_out,
             void* stream);

/* replaces n_substeps x sim.step() followed by reading data.sensordata / data.contact
 * (manenv.py:48-49,65-85).  Device pointers, any may be NULL:
 *   sens_out  [n_envs][nsensordata] f64, the sensordata after the last substep
 *   flags_out [n_envs] int32, OR of SG_FLAG_* raised during the call; an env that raised
 *             BADQPOS/BADQVEL/BADQACC stops integrating for the rest of the call
 *   touch_out [n_envs] int32, bit (2*chain + box) set when that finger box is in contact
 *             with an object geom in the final contact list (data.contact at read time)
 * sens_stride: element stride between envs in sens_out (0 = nsensordata); lets the caller
 * write step t of a [n_envs][T][nsensordata] block directly. */
int sg_step(sg_batch* b, int n_substeps, double* sens_out, long long sens_stride, int32_t* flags_out, int32_t* touch_out,
            void* stream);

/* state access for tests and checkpointing: [n_envs][nq] (qpos), [n_envs][nv] (qvel, qacc_warmstart) and
 * [n_envs][nu] (act, ctrl); device pointers, any may be NULL.  A free joint's seven positions are the body's world position and
 * quaternion, its six velocities the linear velocity in the world frame and the angular velocity in the body frame (MuJoCo's layout). */
int sg_get_state(sg_batch* b, double* qpos, double* qvel, double* act, double* qacc_warmstart, double* ctrl, void* stream);
int sg_set_state(sg_batch* b, const double* qpos, const double* qvel, const double* act, const double* qacc_warmstart,
                 const double* ctrl, void* stream);

/* diagnostics of the last sg_step/sg_reset: [n_envs] int32 each, device pointers, may be NULL:
 * number of contacts, constraint rows and PGS sweeps of the final substep */
int sg_get_solver_stats(sg_batch* b, int32_t* ncon, int32_t* nefc, int32_t* iters, void* stream);

/* kernel pipeline (same results to round-off, all parity-tested): 3 = tree (csrc/sg_tree.h: one env per wavefront, state in LDS;
 * the only pipeline for grippers outside the two-finger class -- any number of serial finger chains up to 24 dofs, multi-site
 * tendons, limited sliders: the reference's soft_grip_four_fingers.xml -- and for an object on a free joint: the reference's
 * soft_experiments_softball.xml; selectable for fix-rows-only two-finger models),
 * 2 = rows (default for the two-finger class: chain / phase / row-parallel PGS
 * kernels, a lane quad per finger stream in the solver), 1 = split (same chain with one lane per finger stream),
 * 0 = fused (one kernel per call, everything on chip).  The env var SG_PIPELINE=fused|split|rows sets the default of
 * new batches.  A model compiled with the composite's neighbour equalities (two-joint equality rows, eq_obj2id >= 0;
 * softgrip_model.h, mjcf.py composite_neighbors=True) runs in the rows pipeline only: its batches start there and
 * sg_set_pipeline(b, 0 or 1) returns SG_ERR_MODEL. */
int sg_set_pipeline(sg_batch* b, int pipeline);

/* Contact read-out for grippers with more than 32 finger boxes (the four-finger gripper has 64; replaces the loop over
 * data.contact of manenv.py:65-85): out [n_envs][nwords] int32, bit g of an env's words (word g / 32, bit g % 32) set when moving
 * finger box g -- the model's box geoms on moving bodies in geom-id order -- touches an object geom in the contact list of the
 * last sg_step / sg_reset.  Word 0 equals touch_out for models with up to 32 boxes.  (Fused pipeline: valid when the call passed
 * touch_out = NULL.)  sg_model_nboxes: the number of such boxes. */
int sg_get_touch_words(sg_batch* b, int32_t* out, int nwords, void* stream);
int sg_model_nboxes(const sg_model* m);

/* envs per wavefront of the rows pipeline's solver kernel: 8 fills the wavefront (fix-rows-only models, chosen automatically from
 * 8185 envs on, where 8 per wavefront still give every SIMD of the chip a wavefront), 4 spreads a smaller batch over twice as many
 * wavefronts.  Same results either way (parity-tested in both).  epw: 0 = automatic, 4, 8; SG_ERR_MODEL for 8 on a model with
 * neighbour equality rows (always 4).  sg_solver_envs_per_wavefront reports what the next sg_step will use. */
int sg_set_solver_envs_per_wavefront(sg_batch* b, int epw);
int sg_solver_envs_per_wavefront(const sg_batch* b);

/* tree pipeline: how many workgroups (= envs, one wavefront each) of this batch's kernel the runtime places on one CU with the LDS the
 * launch asks for (hipOccupancyMaxActiveBlocksPerMultiprocessor) -- what bench.py reports as config.tree_workgroups_per_cu.
 * 0 for a batch that does not run the tree pipeline; negative: an error code. */
int sg_tree_workgroups_per_cu(const sg_batch* b);

/* ---- pose read-out: replaces reading data.xpos / data.xquat / data.geom_xpos / data.geom_xmat after mj_kinematics.
 * mj_kinematics for the listed envs: [n_ids][nbody][3|4] body xpos / xquat, [n_ids][ngeom][3|9] geom_xpos / geom_xmat (row-major).
 * env_ids: HOST pointer to n_ids env indices (NULL: all envs in order, n_ids == n_envs); outputs: device pointers, any may be NULL.
 * Reads the batch's current qpos and changes nothing in it; an env whose qpos holds a NaN or inf gets NaN poses. */
int sg_get_poses(sg_batch* b, const int32_t* env_ids, int n_ids, double* xpos, double* xquat, double* geom_xpos, double* geom_xmat, void* stream);
int sg_model_nbody(const sg_model* m);
int sg_model_ngeom(const sg_model* m);

/* ---- headless renderer (no window, no GL; replaces MjViewer's picture, manenv.py:114-116).  Every geom is drawn as its own primitive
 * (plane, sphere, capsule, box; a model with another geom type fails with SG_ERR_MODEL) with a fixed shading.
 * cam[7]: MuJoCo's free camera = lookat xyz, distance, azimuth, elevation, fovy (degrees, vertical); forward =
 * (cos el cos az, cos el sin az, sin el), eye = lookat - distance forward, up = +z.
 * sg_model_default_camera: a camera that frames the scene at qpos0 (host only, needs no device).
 * sg_render: ray-cast images of the listed envs, device pointers, any may be NULL:
 *   rgba  [n_ids][height][width][4] uint8, depth [n_ids][height][width] f32 (distance along the optical axis, +inf = background),
 *   segid [n_ids][height][width] int32 (geom id, -1 = background).  Reads the batch's current state; changes nothing in it.
 *   An env whose qpos holds a NaN or inf renders as background.  env_ids as in sg_get_poses. */
int sg_model_default_camera(const sg_model* m, double cam[7]);
int sg_render(sg_batch* b, const double* cam, const int32_t* env_ids, int n_ids, int width, int height,
              uint8_t* rgba, float* depth, int32_t* segid, void* stream);

/* ---- the soft object's skin: what a camera sees of a <composite> with a <skin> child is a surface, not its collision capsules.
 * A skin is triangles bound to bodies, held by the model next to its kinematics table and NOT part of the blob: nvert <= 256 vertices,
 * each with a body id vert_body[v] and a position vert_pos[v][3] in that body's frame; nface <= 512 triangles face[f][3] of vertex
 * indices, front side counter-clockwise; one rgba[4] (alpha is ignored: output alpha stays 255).  Host pointers, no device needed.
 * The model of a scene compiled from MJCF carries the composite's skin (one vertex per shell element at (0, 0, inflate), the six sides'
 * quads split in two; built as at subgrid = 0, textures and materials are not drawn); a model made from a blob has none until it is set.
 * Setting a skin validates before it stores anything: SG_ERR_INVALID for NULL arrays with positive counts, a body id outside
 * [0, nbody), a face index outside [0, nvert), a face that repeats an index, non-finite positions or rgba; SG_ERR_MODEL beyond the
 * limits; a rejected call leaves the old skin in place.  nvert == 0 removes the skin.  Batches of the model pick a new skin up at
 * their next render.  Reading a skin: the sizes always, the arrays where the pointer is not NULL. */
int sg_model_set_skin(sg_model* m, int nvert, const int32_t* vert_body, const double* vert_pos,
                      int nface, const int32_t* face, const float rgba[4]);
int sg_model_skin(const sg_model* m, int* nvert, int* nface, int32_t* vert_body, double* vert_pos,
                  int32_t* face, float* rgba);

/* The renderer with flags.  flags == 0: exactly what the plain call does (same kernels, same bits).  SG_RENDER_SKIN on a model with a skin:
 * the skin is drawn and the geoms of the bodies its vertices are bound to are not; everything else is drawn as before (the
 * composite's centre sphere too).  Skin pixels report segid == ngeom.  Front faces only; a ray through a shared edge or vertex of two
 * triangles hits one of them; of equal distances the smaller face index wins and a geom wins against a triangle.  The shading normal
 * is interpolated from area-weighted vertex normals.  With the flag and no skin: the plain call.  Unknown flag bits: SG_ERR_INVALID. */
enum { SG_RENDER_SKIN = 1 };
int sg_render_ex(sg_batch* b, const double* cam, const int32_t* env_ids, int n_ids, int width, int height,
                 int flags, uint8_t* rgba, float* depth, int32_t* segid, void* stream);

/* ---- contact read-out: replaces the loop `for i in range(data.ncon): data.contact[i]` (manenv.py:65-85).
 * mj_collision for the listed envs at the batch's CURRENT qpos -- what sim.forward(); sim.data.contact[:ncon] would hold: the oracle's
 * candidate pairs, order, bounding tests, narrowphase and cap.  Geometry only (no forces, no solver parameters).  Device pointers, any
 * may be NULL:
 *   ncon  [n_ids] int32: the number of contacts mj_collision keeps for the env (at most the model's nconmax when positive, and 512); it
 *         MAY EXCEED max_contacts; -1 for an env whose qpos holds a NaN or inf (or whose geom poses leave +-1e10);
 *   geom  [n_ids][max_contacts][2] int32: geom1, geom2 in mj_collideGeoms' by-type order (plane < sphere < capsule < box);
 *   dist  [n_ids][max_contacts], pos [n_ids][max_contacts][3], frame [n_ids][max_contacts][9] (normal geom1 -> geom2 in the first row,
 *         completed as mju_makeFrame; the first tangent of a plane - capsule contact follows the capsule's axis).
 * The arrays receive the first min(ncon, max_contacts) contacts in mj_collision's order; slots past that are NOT written (the call does
 * not clear the buffers).  env_ids as in sg_get_poses.  Reads the batch and changes nothing in it; does not synchronise the host.
 * After sg_step the batch's qpos is one Euler integration PAST the collision pass whose list produced touch_out, so this is the NEXT
 * forward pass's list; directly after sg_reset(..., sim_start = 0, ...) or sg_set_state nothing lies between the two and the touch
 * bits recomputed from this list equal sg_get_touch_words.
 * SG_ERR_INVALID (checked before anything touches the device): NULL batch, n_ids <= 0, max_contacts <= 0 with a contact array given, an
 * env id out of range.  sg_model_ncollision_pairs: the candidate geom pairs after the static filters (contype / conaffinity, weld group,
 * parent - child), which the kernel's broadphase walks for every env. */
int sg_get_contacts(sg_batch* b, const int32_t* env_ids, int n_ids, int max_contacts,
                    int32_t* ncon, int32_t* geom, double* dist, double* pos, double* frame, void* stream);
int sg_model_ncollision_pairs(const sg_model* m);

/* ---- ray queries: replaces mj_ray / the rangefinder sensor -- "what lies along this line, and how far away".
 * mj_ray for the listed envs at the batch's CURRENT qpos, n_rays rays per env, in fp64.
 *   origin, dir  device: [n_rays][3], the same rays for every listed env, or [n_ids][n_rays][3] with SG_RAY_PER_ENV in `flags`.
 *                Directions are normalised by the call.
 *   ray_body     HOST, [n_rays], NULL = all -1.  ray_body[r] >= 0: origin and direction of ray r are given in that body's frame and
 *                follow the body's pose in each env; -1: the world frame.
 *   ray_exclude  HOST, [n_rays], NULL = all -1.  ray_exclude[r] >= 0: the geoms of that body are no candidates (mj_ray's bodyexclude:
 *                what a rangefinder does with its own body).
 *   cat_mask     bit c set: the geoms of category c are candidates (mj_ray's geomgroup).  The categories are those of the kinematics
 *                table: the ground plane, static geoms, moving finger boxes, the soft object's shell elements, its centre sphere.
 *   max_dist     <= 0: unlimited; otherwise a hit farther away is a miss.
 * Per-ray rules (the renderer's): only ENTRY hits count -- the smallest t > 0 at which the ray enters a geom from outside.  An origin
 * inside a geom therefore does not see that geom: THIS DEPARTS FROM mj_ray, which reports the exit; a depth probe that starts inside
 * its own (excluded) body and crosses it sees what lies in front, and a surface that has pushed past the origin is not reported from
 * behind.  Planes are one-sided (seen from their +z side).  Of equal distances the smaller geom id wins.  Primitives: plane, sphere,
 * capsule, box; a model with another geom type fails with SG_ERR_MODEL, as sg_render does (and beyond its 320 geoms).
 * Outputs, device pointers, any may be NULL:
 *   dist   [n_ids][n_rays] f64, metres along the unit direction; -1 for a miss;
 *   geomid [n_ids][n_rays] int32; -1 for a miss;
 *   normal [n_ids][n_rays][3] f64: the outward unit normal at the hit, world axes; zeros for a miss.
 * A ray whose direction has zero length or a non-finite component is a miss.  An env whose qpos holds a NaN or inf gets dist = NaN,
 * normal = NaN and geomid = -1.  env_ids as in sg_get_poses.  Reads the batch and changes nothing in it; does not synchronise the host
 * (the two host id arrays are read before the call returns and uploaded with a copy on `stream`).  As for sg_get_contacts: after
 * sg_step the batch's qpos is one Euler integration PAST the collision pass behind touch_out.
 * SG_ERR_INVALID (checked before anything touches the device): NULL batch, origin or dir; n_ids <= 0 or n_rays <= 0; an env id out of
 * range; a body id outside [-1, nbody); cat_mask outside [1, 31]; unknown flag bits; a max_dist that is not finite.
 * Two kernel layouts serve the call (a lane per ray; the lanes of a wavefront over the geoms of one ray), chosen from n_rays; the env
 * var SG_RAY_LAYOUT=rays|geoms, read per call, forces one.  Both give the same bits.
 * SG_RAY_SKIN in `flags`, on a model with a skin (sg_model_set_skin): the rays see the soft object as the surface the renderer draws
 * with SG_RENDER_SKIN and not as its collision capsules.
 *   candidates   the skin's triangles when cat_mask holds SG_RAY_ELEM.  The geoms of the bodies the skin's vertices are bound to are
 *                NEVER candidates, whatever cat_mask says (the renderer's hidden geoms).  Everything else, the centre sphere included,
 *                is as without the flag.  ray_exclude[r] = body also removes every triangle with a vertex bound to that body.
 *   vertices     xpos[body] + R(xquat[body]) vert_pos in fp64, from this call's poses.
 *   hit          front faces only (counter-clockwise seen from outside): with a, b, c relative to the origin and n = (b - a) x (c - a),
 *                n . d < 0 and t = (n . a) / (n . d) > 0 -- the entry-hit rule, so an origin inside the closed skin sees nothing of it.
 *                A triangle seen edge-on is a miss; a hit beyond max_dist is a miss.
 *   geomid       ngeom + face index: geomid >= ngeom means "skin, triangle geomid - ngeom".  The order is the one above -- smaller
 *                distance, then smaller id -- so a geom wins a tie against a triangle and the smaller face index among triangles.
 *   normal       the triangle's unit face normal n / |n|, world axes: flat, NOT interpolated (a distance sensor).
 *   watertight   a ray that crosses the closed skin from outside hits it, also when it passes exactly through a shared edge or a
 *                vertex: an edge's value is computed once, the endpoint of smaller vertex index first, from the vertices' coordinates in a
 *                frame built from the ray direction, with an exact sign; zero counts as inside.
 * An env with a pose or a vertex that is not finite gets NaN, NaN, -1 as above.  With the flag on a model WITHOUT a skin, or without
 * the flag, the call is exactly the plain one: the same kernels, the same launch, the same bits.  Primitives beside the skin: as above. */
enum { SG_RAY_GROUND = 1, SG_RAY_STATIC = 2, SG_RAY_FINGER = 4, SG_RAY_ELEM = 8, SG_RAY_CENTER = 16, SG_RAY_ALL = 31 };   /* cat_mask */
enum { SG_RAY_PER_ENV = 1, SG_RAY_SKIN = 4 };   /* flags (bit 2 is not assigned: SG_ERR_INVALID, as every unknown bit) */
int sg_ray(sg_batch* b, const int32_t* env_ids, int n_ids, int n_rays, const double* origin, const double* dir,
           const int32_t* ray_body, const int32_t* ray_exclude, int cat_mask, double max_dist, int flags,
           double* dist, int32_t* geomid, double* normal, void* stream);

/* ---- velocity, tendon and energy read-outs: replaces reading data.cvel / mj_objectVelocity, data.ten_length / data.ten_velocity and
 * data.energy after mj_forward.  Pure functions of the batch's CURRENT qpos and qvel and of its per-env stiffness; one kernel walks the
 * kinematic tree once per call, whichever of the three is asked.  Common to all three: env_ids as in sg_get_poses (HOST, NULL = all);
 * outputs are device pointers, any may be NULL; the calls read the batch, change nothing in it and do not synchronise the host; an env
 * whose qpos or qvel holds a NaN or inf gets NaN in every output and disturbs no other env.  No atomics: two calls give the same bits,
 * and an env's bits do not depend on which envs are listed beside it or in what order.
 * SG_ERR_INVALID (checked before anything touches the device): NULL batch, n_ids <= 0, an env id out of range.  SG_ERR_MODEL: a model the
 * pose read-out cannot run, a tendon with wraps other than joints only or sites only, and a model of more than 627 bodies (a body's pose
 * and twist are 13 doubles of the kernel's LDS block, which stays within 64 KB).
 *
 * Velocities: ang, lin, com_lin [n_ids][nbody][3] each, world axes.  ang: the body's angular velocity.  lin: the linear velocity of the
 *   body frame's origin, the point xpos that sg_get_poses reports.  com_lin: the linear velocity of the body's centre of mass
 *   xpos + R body_ipos.  Body 0 (the world) is zero.  THE DEFINING PROPERTY: the outputs are the time derivative of what sg_get_poses
 *   returns when qpos moves the way qvel says (mj_integratePos) -- slide and hinge joints at rate qvel; a free joint's position at its
 *   three linear components (world frame) and its quaternion at 1/2 q (0, w), w the three angular components in the BODY frame (the
 *   layout sg_get_state documents).  The joints of a body are taken in joint order, each hinge about its anchor as mj_kinematics places
 *   it.  The velocity of any point p fixed on a body: lin + ang x (p - xpos).
 * Tendons: length, velocity [n_ids][ntendon].  A fixed tendon: sum of coef q and of coef qvel over its joint wraps.  A spatial tendon
 *   (site wraps): the sum of the site-to-site segment lengths at this call's poses and its time derivative, the sum over segments of
 *   unit segment . (v_next - v_prev); a segment shorter than 1e-15 counts its length and no velocity.
 * Energy: energy [n_ids][4] = gravity, joint springs, tendon springs, kinetic (MuJoCo's data.energy: the sum of the first three, the
 *   fourth).  Gravity: minus the sum over bodies >= 1 of m g . xipos.  Joint springs: the sum of 1/2 k (q - qpos_spring)^2 over slide and
 *   hinge joints (a free joint has none).  Tendon springs: the sum of 1/2 k (L - tendon_lengthspring)^2.  k is what the next sg_step
 *   would use for this env: its sg_set_stiffness value on the listed joints and tendons, the model's own elsewhere; ordering is stream
 *   ordering, so a call after sg_set_stiffness with a device k on the same stream sees the new k.  Kinetic:
 *   1/2 sum over bodies of (m |com_lin|^2 + w' R I R' w), I = body_imat about the centre of mass, plus 1/2 sum of dof_armature qvel^2:
 *   1/2 qvel' M qvel with the mass matrix of mj_crb. */
int sg_get_velocities(sg_batch* b, const int32_t* env_ids, int n_ids, double* ang, double* lin, double* com_lin, void* stream);
int sg_get_tendons(sg_batch* b, const int32_t* env_ids, int n_ids, double* length, double* velocity, void* stream);
int sg_get_energy(sg_batch* b, const int32_t* env_ids, int n_ids, double* energy, void* stream);

/* ---- mass-matrix, joint-force and inverse-dynamics read-outs: replaces reading data.qM (through mj_fullM), data.qfrc_bias,
 * data.qfrc_passive and data.qfrc_actuator after mj_forward, and calling mj_inverse for data.qfrc_inverse.  Pure functions of the batch's
 * CURRENT qpos, qvel and act and of its per-env stiffness; one kernel walks the kinematic tree out and back once per call, whichever of
 * the three is asked.  Common to all three, exactly as for sg_get_velocities: env_ids is a HOST pointer (NULL = all); outputs are device
 * pointers, any may be NULL -- qacc alone, a device pointer to [n_ids][nv] (row k belongs to the k-th listed env), is required; the
 * calls read the batch, change nothing in it and do not synchronise the host; free quaternions are normalised on the way in; an env
 * whose qpos or qvel (for sg_inverse_dynamics also: whose qacc row) holds a NaN or inf gets NaN in every output and disturbs no other
 * env.  No atomics: two calls give the same bits, and an env's bits depend neither on which envs are listed beside it, nor on their
 * order, nor on which outputs are NULL.
 * SG_ERR_INVALID (checked before anything touches the device): NULL batch, n_ids <= 0, an env id out of range, NULL qacc.
 * SG_ERR_MODEL, with the limit named in the message: a model the velocity read-out cannot run, and a model of more than 449 bodies, 1024
 * dofs or 128 tendons (a body takes 29 doubles, a dof 7 and a tendon 2 of the kernel's LDS block, which stays within the 160 KB a
 * workgroup can have).
 *
 * The dofs follow sg_get_velocities' conventions: a slide or hinge dof moves along / turns about its joint's axis as mj_kinematics
 * places it; a free joint's three linear dofs move the body along the WORLD axes, its three angular dofs turn it about the BODY's own
 * axes through the body frame's origin.
 * M: [n_ids][nv][nv], row-major, dense: mj_fullM(data.qM).  M = sum over bodies of (m Jp' Jp at the centre of mass + Jr' R I R' Jr)
 *   + diag(dof_armature), Jp and Jr the body's translational and rotational Jacobians over the dofs above.  EVERY entry is written, the
 *   zeros included (dofs of which neither is an ancestor of the other), so the buffer need not be cleared; each pair is computed once
 *   and stored twice: M is symmetric to the bit.  nv * nv * 8 bytes per env: list fewer envs per call where memory is short.
 * bias: [n_ids][nv], data.qfrc_bias: recursive Newton-Euler at qacc = 0 -- Coriolis, centrifugal and gravity terms -- on the left-hand
 *   side, M qacc + bias = applied forces; at rest it is PLUS the gradient of sg_get_energy's gravity term.
 * passive: [n_ids][nv], data.qfrc_passive: joint springs -k (q - qpos_spring) (slide and hinge; a free joint has none), joint dampers
 *   -dof_damping qvel, and the tendons' sum over tendons of J_t' (-k_t (L - tendon_lengthspring) - tendon_damping Ldot), J_t the
 *   gradient of sg_get_tendons' length.  k is what the next sg_step would use for this env, as in sg_get_energy; stream ordering
 *   against sg_set_stiffness likewise.  The tendon damper is reported as this force WHETHER OR NOT the model integrates it implicitly
 *   (tendon_damper = implicit): the flag changes how sg_step advances the velocity, not what force acts at the current state.
 * actuator: [n_ids][nv], data.qfrc_actuator: sum over actuators u of gear J_t' (gain act + bias0 + bias1 gear L + bias2 gear Ldot), t
 *   the actuator's tendon, act the batch's CURRENT activation (sg_get_state's), as mj_forward's actuation stage has it.
 * qfrc_inverse: [n_ids][nv] = M qacc + bias - passive, MuJoCo's definition (mj_inverse), for the acceleration the caller gives: what all
 *   other forces together -- actuators, contacts, equalities -- must have applied to produce it.  Computed as ONE Newton-Euler pass
 *   with the given acceleration (plus dof_armature qacc), not as a product with a formed M.  With the qacc of a step,
 *   qfrc_inverse - actuator is the generalised force of the constraints. */
int sg_get_mass_matrix(sg_batch* b, const int32_t* env_ids, int n_ids, double* M, void* stream);
int sg_get_joint_forces(sg_batch* b, const int32_t* env_ids, int n_ids, double* bias, double* passive, double* actuator, void* stream);
int sg_inverse_dynamics(sg_batch* b, const int32_t* env_ids, int n_ids, const double* qacc, double* qfrc_inverse, void* stream);

/* ---- point motion and point Jacobians: replaces mj_jac / mj_jacBody / mj_jacSite, reading data.cacc or calling mj_objectVelocity /
 * mj_objectAcceleration, and declaring a gyro or an accelerometer at a site in the MJCF: both can be asked of ANY body-fixed point, at
 * run time, without touching the model.
 * A POINT (probe) is pt_body[p] in [0, nbody) -- body 0, the world, is allowed --, pt_pos[p][3], a position in that body's frame, and
 * optionally pt_quat[p][4], the probe's frame relative to the body's (a NULL array: identity; the call normalises each quaternion).  A
 * point given a site's site_bodyid, site_pos and site_quat IS that site: sg_model_nsite / sg_model_sites hand the model's sites out in
 * that form (host arrays of nsite, nsite x 3 and nsite x 4 entries, any may be NULL).  The point arrays are HOST pointers, as sg_ray's
 * ray_body: they are read before the call returns and reach the device by a copy on `stream`.
 * State: env_ids as in sg_get_poses (HOST, NULL = all).  qpos [n_ids][nq], qvel [n_ids][nv] and qacc [n_ids][nv] are DEVICE pointers,
 * row k belonging to the k-th listed env; a NULL qpos or qvel means the batch's CURRENT qpos or qvel, a NULL qacc means zero.  The
 * calls read the batch, change nothing in it and do not synchronise the host; free quaternions are normalised on the way in.
 * Outputs: device pointers, any may be NULL, world axes unless stated.
 *   pos   [n_ids][n_pts][3]  the point; mat [n_ids][n_pts][9] the probe's frame, row-major: R(xquat[body]) R(pt_quat).
 *   vel   [n_ids][n_pts][6]  the body's angular velocity, then the linear velocity of the material point: lin + ang x (p - xpos) in
 *                            sg_get_velocities' terms.
 *   acc   [n_ids][n_pts][6]  the body's angular acceleration, then the acceleration of the material point; kinematic, WITHOUT
 *                            gravity: J qacc + Jdot qvel.
 *   gyro  [n_ids][n_pts][3]  mat' ang; accel [n_ids][n_pts][3] = mat' (a_point - gravity): what MuJoCo's gyro and accelerometer at a
 *                            site of that pose read.  A probe on the world reads minus gravity.
 *   jacp, jacr [n_ids][n_pts][3][nv]  mj_jac's layout: column d is dof d's effect on the point under sg_get_velocities' dof
 *                            conventions -- a slide dof gives (u, 0), a hinge dof (u x (p - anchor), u), a free joint's linear dofs act
 *                            along the WORLD axes, its angular dofs about the BODY's own axes through xpos.  EVERY entry is written,
 *                            the zeros included (a dof whose body is neither the point's body nor one of its ancestors), so the
 *                            buffers need not be cleared.  vel = (jacr qvel, jacp qvel).
 * No atomics: two calls give the same bits; an env's bits depend neither on the env list, nor on its order, nor on which outputs are
 * NULL; a point's bits depend neither on n_pts nor on its place in the list.  An env whose qpos, qvel or qacc row -- those the call
 * uses: the given one, or the batch's current one where none is given; sg_get_jacobians uses qpos alone -- holds a NaN or inf gets NaN
 * in every output of the call (every entry of its Jacobians) and disturbs no other env.
 * SG_ERR_INVALID (checked before anything touches the device; nothing is written): NULL batch, n_ids <= 0, an env id out of range,
 * n_pts <= 0, NULL pt_body or pt_pos, a body id outside [0, nbody), a non-finite pt_pos or pt_quat, a pt_quat of zero length.
 * SG_ERR_MODEL, with the limit named in the message: a model the velocity read-out cannot run -- its tables are walked here, so its
 * 627 bodies are the body limit a caller meets -- and a model of more than 1024 dofs.  (The kernel's own LDS block, 19 doubles a body,
 * 7 doubles and an int a dof within the 160 KB a workgroup can have, would hold 672 bodies: a check that stands behind the first and
 * is reached only if that one is ever raised.)
 *
 * THE EXACT VIRTUAL IMU.  After sg_step, sensordata belongs to the LAST substep's forward pass; the batch's qpos and qvel are one
 * integration past that pass, and qacc_warmstart is that pass's qacc.  So, for an env step of n substeps:
 *   sg_step(n - 1); sg_get_state(qpos, qvel) into buffers of the caller; sg_step(1);
 *   sg_get_state(qacc_warmstart); sg_get_point_motion(qpos = saved, qvel = saved, qacc = qacc_warmstart)
 * gives gyro / accel of the same forward pass as that step's sensordata -- at the model's own sites they equal it -- at any point.
 * No sg_set_state is involved and the batch is never written. */
int sg_get_point_motion(sg_batch* b, const int32_t* env_ids, int n_ids, int n_pts, const int32_t* pt_body, const double* pt_pos, const double* pt_quat,
                        const double* qpos, const double* qvel, const double* qacc, double* pos, double* mat, double* vel, double* acc, double* gyro,
                        double* accel, void* stream);
int sg_get_jacobians(sg_batch* b, const int32_t* env_ids, int n_ids, int n_pts, const int32_t* pt_body, const double* pt_pos, const double* qpos, double* jacp,
                     double* jacr, void* stream);
int sg_model_nsite(const sg_model* m);
int sg_model_sites(const sg_model* m, int32_t* body, double* pos, double* quat);   /* host pointers, any may be NULL */

/* ---- mass-matrix solves, smooth forward dynamics and point inertias: replaces mj_solveM, reading data.qacc_smooth / data.qfrc_smooth
 * after mj_fwdAcceleration, and forming J M^-1 J' on the host from a downloaded M.  Everything here starts with the inverse of M, the
 * matrix sg_get_mass_matrix documents (same dof conventions, armature included); M itself never leaves the chip: only its nonzero
 * entries -- (i, j) with j = i or an ancestor dof of i -- are formed, and factorised in place in LDS.
 * Each call is a pure function of the batch's CURRENT qpos (sg_forward_smooth: and qvel, act and the per-env stiffness the env's next
 * step uses, in stream order against sg_set_stiffness).  env_ids as in sg_get_poses (HOST, NULL = all); all other arrays are DEVICE
 * pointers unless stated, row k belonging to the k-th listed env.  The calls read the batch, change nothing in it and do not
 * synchronise the host; free quaternions are normalised on the way in.
 * The factorisation is mj_factorM's: M = L' D L, L unit lower triangular with L[k][j] != 0 only where dof j is an ancestor of dof k.  NO
 * pivoting and NO clamping of small pivots.
 * pivot: [n_ids], min over the dofs of D_i / M_ii: 1 for a diagonal M, falling towards 0 as M approaches singularity.  If some D_i is not
 *   finite or is <= 0 the env gets NaN in every other output of the call and pivot holds that ratio (or NaN).  A tiny positive pivot gives
 *   finite results that are not meaningful: pivot is how the caller learns of it.
 * sg_solve_mass: x = M^-1 y (mj_solveM).  y and x are [n_ids][n_rhs][nv]; x may be the same pointer as y.  y and at least one of x and
 *   pivot are required.
 * sg_forward_smooth: qfrc_smooth [n_ids][nv] = passive + actuator + qfrc_applied - bias, sg_get_joint_forces' three arrays and the
 *   caller's qfrc_applied [n_ids][nv] (NULL: zero); qacc_smooth [n_ids][nv] = M^-1 qfrc_smooth (mj_fwdAcceleration): the acceleration
 *   without contacts, equalities and limits.  Any output may be NULL.  Two identities: sg_inverse_dynamics(qacc_smooth) = actuator +
 *   qfrc_applied; and with the qacc of a step, M (qacc - qacc_smooth) is the generalised force of the constraints.
 * sg_get_point_inertia: W [n_ids][n_pts][6][6] = J M^-1 J', the inverse inertia seen at a body-fixed point: J is jacr in rows 0 - 2 and
 *   jacp in rows 3 - 5 of sg_get_jacobians for the same points -- the angular-then-linear order of sg_get_point_motion's vel.  Each pair
 *   is computed once and stored twice: W is symmetric to the bit; all zeros for a point on the world body.  1 / (n' W[3:6][3:6] n) is
 *   the effective mass along a unit vector n.  pt_body [n_pts] and pt_pos [n_pts][3] are HOST arrays as in sg_get_jacobians.
 * No atomics: two calls give the same bits; an env's bits depend neither on the env list, nor on its order, nor on which outputs are
 * NULL; a right-hand side's bits depend neither on n_rhs nor on its place in the list, a point's neither on n_pts nor on its place.  An
 * env whose state -- the qpos, qvel, y rows or qfrc_applied row that the call uses -- holds a NaN or inf gets NaN in every output of the
 * call, pivot included, and disturbs no other env.
 * SG_ERR_INVALID (checked before anything touches the device; nothing is written): NULL batch, n_ids <= 0, an env id out of range,
 * n_rhs <= 0 or n_pts <= 0, NULL y, NULL x and pivot together, NULL pt_body or pt_pos, a body id outside [0, nbody), a non-finite pt_pos.
 * SG_ERR_MODEL, with the limit named in the message: a model sg_get_mass_matrix cannot run, and a model whose LDS block does not fit
 * the 160 KB a workgroup can have: sg_get_mass_matrix' records, nM + nv doubles of factor (nM: the nonzero entries of M's lower
 * triangle) and six right-hand sides of nv doubles.  A serial chain of 1024 dofs has nM = 524 800 and is refused; the committed scenes
 * have nM between 54 and 1567. */
int sg_solve_mass(sg_batch* b, const int32_t* env_ids, int n_ids, int n_rhs, const double* y, double* x, double* pivot, void* stream);
int sg_forward_smooth(sg_batch* b, const int32_t* env_ids, int n_ids, const double* qfrc_applied, double* qacc_smooth, double* qfrc_smooth, double* pivot,
                      void* stream);
int sg_get_point_inertia(sg_batch* b, const int32_t* env_ids, int n_ids, int n_pts, const int32_t* pt_body, const double* pt_pos, double* W, double* pivot,
                         void* stream);

/* ---- constraint and contact forces: replaces reading data.efc_force / data.qfrc_constraint / data.qacc after sim.forward() and
 * mj_contactForce.  sg_get_forces is mj_forward's constraint stage at the batch's CURRENT state -- qpos, qvel, act, ctrl,
 * qacc_warmstart and the per-env stiffness, in stream order against sg_set_stiffness and sg_set_state: what the env's next forward pass
 * will compute (after sg_step: the NEXT pass's forces, as with sg_get_contacts).  It reads the batch and changes nothing in it --
 * qacc_warmstart is not updated -- and does not synchronise the host.  env_ids as in sg_get_poses (HOST, NULL = all); every other array
 * is a DEVICE pointer, row k belonging to the k-th listed env, and any may be NULL.
 * Rows, in mj_makeConstraint's order: equalities by id (one- and two-joint polynomial equalities, tendon equalities); joint limits by
 * joint id, lower side first, only where dist < margin; contacts in sg_get_contacts' order, only those with dist < includemargin, one
 * row for condim 1 and three for condim 3 (elliptic cones).  Contact parameters are mixed as mj_contactParam does at equal priority;
 * impedance, R and the reference acceleration as mj_makeImpedance (refsafe, impratio); njmax and nconmax cut the list as mj_forward does.
 * The solver is mj_solPGS from mj_forward's warm start, with its early exit.
 *   nefc, iters, ncon  [n_ids]: rows, sweeps run, contacts.  nefc may exceed max_rows.  nefc = ncon = -1 for an env whose state holds a
 *                      NaN or inf (or whose mass matrix has a pivot that is not positive): such an env gets NaN in every double output
 *                      and disturbs no other env
 *   efc_type, efc_id, efc_force  [n_ids][max_rows]: type 0 equality, 3 limit, 5 frictionless contact, 7 elliptic contact; id the equality,
 *                      the joint, or the contact's index in sg_get_contacts' list.  Only the first min(nefc, max_rows) are written
 *   contact_force      [n_ids][max_contacts][3]: the force of contact i of sg_get_contacts' list in that contact's frame, normal first
 *                      (mj_contactForce's first three numbers): the bits of its efc_force entries; zero for a contact without rows,
 *                      zero tangential parts for condim 1.  Only the first min(ncon, max_contacts) are written
 *   qfrc_constraint    [n_ids][nv] = J' f;   qacc [n_ids][nv] = qacc_smooth + M^-1 J' f, data.qacc after mj_forward
 * sg_model_max_rows: the rows the call reserves per env -- every equality, both sides of every limited joint, three rows per contact
 * the list can hold (cut by njmax).  The call needs about 2 x that x nv doubles per env (the rows' J and M^-1 J'), so the env list is
 * processed in chunks, launched in stream order inside a work space that the batch allocates at the first call and that holds at most
 * sg_set_forces_workspace's bytes (default 256 MiB; SG_ERR_INVALID below one env's need).  No atomics: two calls give the same bits,
 * and an env's bits depend neither on the chunking, nor on the env list or its order, nor on which outputs are NULL.
 * SG_ERR_INVALID (checked before anything touches the device): NULL batch, n_ids <= 0, an env id out of range, max_rows <= 0 with a row
 * array given, max_contacts <= 0 with contact_force given.  SG_ERR_MODEL, with the limit named: a model sg_solve_mass refuses, a condim
 * other than 1 or 3, an equality that is neither a joint nor a tendon equality, a row list that does not fit the 160 KB of LDS. */
int sg_get_forces(sg_batch* b, const int32_t* env_ids, int n_ids, int max_rows, int max_contacts, int32_t* nefc, int32_t* iters, int32_t* efc_type,
                  int32_t* efc_id, double* efc_force, int32_t* ncon, double* contact_force, double* qfrc_constraint, double* qacc, void* stream);
int sg_model_max_rows(const sg_model* m);
int sg_set_forces_workspace(sg_batch* b, size_t bytes);

/* ---- the soft object as one thing: replaces downloading every element body's pose and twist to redo on the host what the renderer and
 * sg_ray do on the chip -- the surface, its volume and width, and the body-tree sums mj_subtreeVel / data.subtree_com give.  The skin is
 * the closed triangle mesh bound to bodies that sg_model_set_skin attaches (SG_RAY_SKIN and SG_RENDER_SKIN show the same vertices).
 * Each call is a pure function of the batch's CURRENT qpos and qvel.  env_ids as in sg_get_velocities (HOST, NULL = all); outputs are
 * DEVICE pointers, row k belonging to the k-th listed env, and any may be NULL.  The calls read the batch, change nothing in it and do
 * not synchronise the host (the first call after sg_model_set_skin uploads the skin's tables again, as sg_render_ex does); free
 * quaternions are normalised on the way in.  An env whose qpos or qvel holds a NaN or inf gets NaN in every double output and -1 in
 * every int output, and disturbs no other env.  No atomics: two calls give the same bits; an env's bits depend neither on the env list,
 * nor on its order, nor on which outputs are NULL; a direction's bits depend neither on n_dirs nor on its place in the list.
 * Host-side model queries (no device):
 *   sg_model_skin_closed   1 when every directed edge (a, b) of the skin's faces occurs once and (b, a) occurs once, else 0; -1 without
 *                          a skin
 *   sg_model_skin_root     the deepest body that is an ancestor of (or is) every body the skin's vertices are bound to, "the object";
 *                          -1 without a skin
 *   sg_model_skin_rest     rest [nvert][3] (HOST): the vertices at qpos0 in frame_body's frame (-1: world)
 *   sg_model_subtree_mass  mass [nbody] (HOST): the mass of every body's subtree, row 0 the whole model's
 * sg_get_skin_vertices: every array is [n_ids][nvert][3].  pos = xpos[body] + R(xquat[body]) vert_pos, the vertex SG_RAY_SKIN documents;
 *   vel = lin + ang x (pos - xpos), the material point's velocity in sg_get_velocities' terms; local = R_f' (pos - xpos_f) in
 *   frame_body's frame (-1: local equals pos).  Any skin, open or closed.
 * sg_get_shape: shape [n_ids][SG_SHAPE_N]: volume V; area A; the centroid of the enclosed solid (3); its central second moments
 *   int (x - c)(x - c)' dV as xx, yy, zz, xy, xz, yz (6); dV/dt.  The integrals are taken about p0, vertex 0's position: for face
 *   (i, j, k) with a, b, c its vertices minus p0, det = a . (b x c) and s = a + b + c: V = sum det / 6, A = sum |(b - a) x (c - a)| / 2,
 *   first moment sum det s / 24, second moment sum det (aa' + bb' + cc' + ss') / 120, dV/dt = sum (va . (b x c) + a . (vb x c) +
 *   a . (b x vc)) / 6 with velocities relative to vertex 0's.  Centroid and central moments follow by one division and one subtraction,
 *   without clamping: V = 0 gives NaN there, and V says why.  shape needs a CLOSED skin (wound outward for V > 0).
 *   dir [n_dirs][3] and dir_body [n_dirs] (NULL: all -1) are HOST arrays, read before return and uploaded on `stream`.  lo, hi
 *   [n_ids][n_dirs]: the min and max over the vertices of d . (pos - o), d the normalised direction -- in world axes with o = 0 for
 *   dir_body -1, else turned with that body and o its xpos: hi - lo is the object's width along a palm-fixed grip axis.  lo_vert, hi_vert
 *   [n_ids][n_dirs]: the vertex attaining it, the smallest index on a tie.  The extents need no closed skin.  n_dirs may be 0 with NULL
 *   arrays and is at most 256.
 * sg_get_subtree: every array is [n_ids][nbody][3].  For body i, the sums over i and its descendants in ascending body order:
 *   com = sum m xipos / M_i; linvel = sum m com_lin / M_i (com_lin: sg_get_velocities'); angmom = sum (R I R' w + m (xipos - com_i) x
 *   com_lin), about the subtree's own com, in world axes.  Row 0 is the whole model.  A subtree with M_i = 0 gets the body's own xipos
 *   and com velocity, and a zero angmom.  Needs no skin.
 * SG_ERR_INVALID (checked before anything touches the device; nothing is written): NULL batch, n_ids <= 0, an env id out of range,
 * frame_body or a dir_body outside [-1, nbody), n_dirs < 0 or above 256, n_dirs > 0 with NULL dir, a direction that is not finite or of
 * zero length.  SG_ERR_MODEL, with the limit named in the message: a model sg_get_velocities cannot run, no skin (the two skin calls),
 * an open skin with shape given, an LDS block -- 22 doubles per body and 6 per vertex -- beyond 160 KB. */
#define SG_SHAPE_N 12
int sg_model_skin_closed(const sg_model* m);
int sg_model_skin_root(const sg_model* m);
int sg_model_skin_rest(const sg_model* m, int frame_body, double* rest);
int sg_model_subtree_mass(const sg_model* m, double* mass);
int sg_get_skin_vertices(sg_batch* b, const int32_t* env_ids, int n_ids, int frame_body, double* pos, double* vel, double* local, void* stream);
int sg_get_shape(sg_batch* b, const int32_t* env_ids, int n_ids, int n_dirs, const double* dir, const int32_t* dir_body, double* shape, double* lo,
                 double* hi, int32_t* lo_vert, int32_t* hi_vert, void* stream);
int sg_get_subtree(sg_batch* b, const int32_t* env_ids, int n_ids, double* com, double* linvel, double* angmom, void* stream);

/* The recurrence of one direction of one fp64 LSTM layer with H = 128 hidden units (csrc/sg_lstm.hip), for the Conv-LSTM and
 * Conv-BiLSTM regressors (soft-grip_amd/lstm.py).  Keras' conventions: gate order i, f, g (the candidate), o along the 4H axis, sigmoid
 * for i, f and o, tanh for g and for the cell, row-major kernels.  The caller keeps what is regular -- the input projection
 * z = x.kernel + bias for all time steps, and the weight gradients as GEMMs over the stored sequences -- and these two calls do what
 * is serial in time, each as ONE kernel launch that walks all T steps with h and c on chip.  They need no batch and no model: all
 * pointers are device pointers on the current device, `stream` is a hipStream_t (NULL: the default stream), and neither call
 * synchronises the host, allocates or keeps anything: U is read row-major as given, straight from L2, with no re-packing and no scratch.
 * No atomics: two runs give the same bits, and a batch row's results do not depend on B.
 *   z      [B][T][4H]  in: x.kernel + bias in CONSUMPTION order (the caller has reversed time for a layer that goes backwards);
 *                      out when save != 0: the activated gates i, f, g, o in place -- what the backward call takes as `gates`;
 *                      left as it was when save == 0
 *   U      [H][4H]     the recurrent kernel: z_t += h_{t-1} . U
 *   h0, c0 [B][H] or NULL (zeros): the state before the first step
 *   h_seq  [B][T][H] or NULL: h after every step, in consumption order;  h_last, c_last [B][H] or NULL: the state after step T - 1
 *   c_seq  [B][T][H]: c after every step; written and required when save != 0, untouched otherwise
 * SG_ERR_INVALID, checked before anything touches the device: B <= 0 or T <= 0, H != 128, NULL z or U, save without c_seq. */
int sg_lstm_forward(int B, int T, int H, double* z, const double* U, const double* h0, const double* c0,
                    double* h_seq, double* h_last, double* c_last, double* c_seq, int save, void* stream);
/* the reverse-time pass of the same direction.  In: `gates` (z after a saving forward call), c_seq and c0 as there, U, and the gradients
 * flowing in: dh_seq [B][T][H] or NULL (zeros), with respect to every h of h_seq, and dh_last [B][H] or NULL, added to step T - 1's.
 * Out: dz [B][T][4H], the gradient with respect to the forward call's input z (the pre-activations), from which the caller forms the
 * weight gradients; dh0, dc0 [B][H] or NULL, the gradient with respect to the initial state.
 * SG_ERR_INVALID as above: B <= 0 or T <= 0, H != 128, NULL gates, c_seq, U or dz. */
int sg_lstm_backward(int B, int T, int H, const double* gates, const double* c_seq, const double* c0, const double* U,
                     const double* dh_seq, const double* dh_last, double* dz, double* dh0, double* dc0, void* stream);

/* kernel timing hook for bench.py: average device time (ms) of one sg_step/sg_reset call's kernels over the
 * calls since the last call with reset != 0, measured with HIP events on the launch
 * stream.  Synchronises the host. */
int sg_profile_enable(sg_batch* b, int enable);
int sg_profile_read(sg_batch* b, int reset, double* avg_ms, long long* launches);
/* the same for the dominant kernel alone: average device time (ms) of one solver-kernel launch (sg_pgs_rows_kernel / sg_pgs_kernel;
 * one per substep) over the calls since the last reset; the split and rows pipelines only (0 launches otherwise) */
int sg_profile_read_solver(sg_batch* b, int reset, double* avg_ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif /* SOFTGRIP_H */
