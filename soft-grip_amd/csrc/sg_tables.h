// sg_tables.h -- the read-outs' per-model tables as one struct, and the one statement of the order they are built in.  sg_model
// (sg_batch.h) has them as its base; the host twins (sg_readout_host.h), the table tests and the sanitizer programs hold the struct
// itself.  sg_tables_build is defined in sg_tables.cpp with the builders it calls.
#pragma once
#include "sg_point.h"    // (sg_smooth.h, sg_dyn.h, sg_readout.h)
#include "sg_forces.h"   // (sg_solve.h)

struct SgHostTables {
  SgKinHost kin;         // kinematics table of sg_get_poses / sg_render
  SgConHost con;         // candidate pairs, margins and bounding radii of sg_get_contacts
  SgDynHost dyn;         // masses, springs, sites and tendons of sg_get_velocities / sg_get_tendons / sg_get_energy
  SgSmoothHost smooth;   // dampers, actuators, child lists and parent dofs of sg_get_mass_matrix / sg_get_joint_forces / sg_inverse_dynamics
  SgPointHost point;     // the dof-parent chain's entries and the sites of sg_get_point_motion / sg_get_jacobians / sg_model_sites
  SgSolveHost solve;     // the packed factor's schedule of sg_solve_mass / sg_forward_smooth / sg_get_point_inertia
  SgForceHost forces;    // equality records, limited joints, solver parameters and opt's numbers of sg_get_forces
};

// every table of the blob, each built on the ones before it: plan and tree (NULL: none) name the geoms' categories, fast says whether
// the plan is the two-finger one.  Each table answers for itself with ok or err; a table another refuses passes that refusal on
void sg_tables_build(const void* blob, size_t nbytes, const SgPlan& plan, const SgTreeDev* tree, bool fast, SgHostTables* T);
