// sg_tree.h -- the TREE pipeline: mj_step for grippers outside the two-finger class (sg_tree_plan.h), one env per wavefront.
//
// What it replaces: the same calls as the fast kernels -- sim.step() / sim.reset() / sim.forward() of reference
// environment/manenv.py:48-61 -- for the reference's four-finger gripper (data/gripper/soft_grip_four_fingers.xml; SURVEY.md 8(f)
// rank 4).  The stages follow the oracle's restatement of mj_forward / mj_step (oracle/sg_oracle.c: kinematics, tendons,
// mass_matrix + factor, collision, make_constraint, rne_bias, the actuation and smooth-acceleration stages, sol_pgs, the sensor
// stage, Euler with implicit joint damping), restructured for the model class:
//   * a dense mass-matrix block per finger chain (<= 24 x 24) with MuJoCo's L'DL, its inverse by columns; the composite's sliders
//     are 1 x 1 blocks;
//   * A = J M^-1 J' is never formed: a constraint row keeps J and W = M^-1 J', the sweep keeps the accelerations a = M^-1 J' f;
//   * the joint-fix / limit rows of the sliders commute among themselves (each touches its own slider): one row per lane; with the
//     composite's neighbour equalities the equality BLOCKS [fix_e, e's neighbour rows] run by the plan's list schedule, 64 blocks a
//     round; a chain's limit rows run serially on one lane per chain; contacts run as one stream per chain (they commute across
//     chains unless they share a slider) or, when they do not, serially in mj_collision's order with the lanes of the wavefront
//     spread over the dofs of the contact's chain block(s);
//   * collision walks the plan's candidate-pair table (SgPlan::gpairs = mj_collision's pair order) 64 pairs at a time:
//     bounding tests per lane, hits ranked by pair index, one lane per hit in the narrowphase (sg_math.h / sg_general.h);
//   * a FREE OBJECT (reference data/gripper/soft_experiments_softball.xml:8: the composite on a body with a free joint) is an object
//     block with an arrow-shaped mass matrix, solved through a 6 x 6 Schur complement in the body's frame; its joint-fix rows run one
//     after the other (every one moves the body), its contacts carry six object columns.
//
// The code is BULK-SYNCHRONOUS: parallel loops over work items (SGT_PAR), single-lane sections (SGT_ONE) and barriers (SGT_SYNC)
// between them; lanes talk through the env's LDS block and its global work space only.  That is what lets tests/emu run the very
// same source on the host (a parallel loop becomes a serial loop, a wavefront sum the identity) against the oracle -- and the
// sanitizers over it.  On the device the env's state lives in LDS for the whole call (all substeps in one launch).
//
// This file is the umbrella: ONE translation unit (sg_tree.hip for gfx950, tests/emu/sg_tree_emu.cpp for the host), cut by stage.  The parts,
// in the order they are included -- each needs only the ones above it:
//   sg_tree_lanes.h              SGT_DEVICE, the bulk-synchronous vocabulary and its host twins, address spaces, the stages' calling convention,
//                                the list of the SGT_X_* knock-outs
//   sg_tree_layout.h             capacities, TreeArgs, the records' field names, Lds + lds_carve, the work space's sizes and offsets
//   sg_tree_chain.h              L'DL of a serial chain and its solves, the scalar row update, 6 x 6 helpers
//   sg_tree_free.h               the free object's equality rows of the sweep
//   sg_tree_sweep.h              tree_sweep: mj_solPGS for one env
//   sg_tree_frame.inc            the stage frame -- the locals every stage and the driver share -- as TEXT (why: its header)
//   sg_tree_stage_dynamics.h     tree_stage_dynamics     kinematics ... smooth accelerations
//   sg_tree_stage_collision.h    tree_stage_collision    the pair walks and the narrowphase
//   sg_tree_stage_constraints.h  tree_stage_constraints  constraint rows, warmstart, the call of tree_sweep
//   sg_tree_stage_finish.h       tree_stage_finish       qacc, sensors, Euler
//   sg_tree_env.h                tree_env: the whole call for one env
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/softgrip.h"
#include "../../include/softgrip_model.h"
#include "sg_general.h"
#include "sg_plan.h"

#include "sg_tree_lanes.h"
#include "sg_tree_layout.h"
#include "sg_tree_chain.h"
#include "sg_tree_free.h"
#include "sg_tree_sweep.h"
#include "sg_tree_stage_dynamics.h"
#include "sg_tree_stage_collision.h"
#include "sg_tree_stage_constraints.h"
#include "sg_tree_stage_finish.h"
#include "sg_tree_env.h"

#if defined(__HIPCC__)
// launchers (sg_tree.hip): the kernel is a translation unit of its own
hipError_t sg_tree_prepare();
int sg_tree_occupancy(int CS, size_t lds_bytes);   // workgroups per CU the runtime grants the instantiation (sg_tree.hip)
hipError_t sg_launch_tree(const sgt::TreeArgs& a, int CS, size_t lds_bytes, hipStream_t s);
#endif
