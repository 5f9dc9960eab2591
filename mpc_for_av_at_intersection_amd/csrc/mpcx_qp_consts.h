// mpcx_qp_consts.h -- constants of the interior-point iteration.  Both solvers must agree on them: the condensed solver
// (mpcx_qp.hip, through mpcx_common.h) and the stage-structured solver (mpcx_qp_stage.h, whose host build in tests/ has no other
// source).  The tests' CPU checker carries the same values.
#pragma once

// fraction of the step to the boundary the interior-point iteration takes.  0.995 in round 1; 0.999 saves 0.8 of 6.1 iterations
// on the closed-loop workload (numpy replica of the iteration over 1280 harvested QPs: mean 6.09 -> 5.27, 99th percentile 13 -> 13,
// max 15 -> 15; 0.9999 is worse again)
#define MPCX_STEP_FRACTION 0.999
#define MPCX_SLACK_FLOOR 0.5    /* starting point of the iteration: s = max(slack, floor), lam = MPCX_LAM0 */
#define MPCX_LAM0 3.0              /* 1 until round 2; with separate step lengths 3 takes the hardest problems of a launch from 23 to 18 iterations (2 / 5: 18 / 17, slower on average) */

/* Active-set polish (round 3; same rule in the condensed solver and in the tests' CPU checker): an interior-point iterate sits ~sqrt(mu) from the optimum
   on weakly active rows, and the low curvature of the input cost (2R = 0.02) amplifies that -- up to 1e-3 on the hard closed-loop
   problems at the reduced-accuracy exit.  Once the iterate is close (mu <= MPCX_POLISH_MU with small residuals, or at any exit) the
   rows with s < lam are taken as the active set and ONE augmented-Lagrangian solve is made on it -- a round whose barrier weights
   are rho on the active rows and 0 elsewhere, with lam_a + rho gap_a as the rows' linear term: the trial pass is the special
   case "no active row".  "Close" is decided at the END of the step that produces the iterate (the new mu is known exactly there, the
   residuals shrink by one minus the step lengths), so that the polish round takes the place of the iterate's first row pass.  The end point is accepted only if it is a KKT point (new multipliers lam_a + rho gap_a' >= 0, no other
   row violated): then it is the minimiser up to |lam - lam*| / rho.  Otherwise rows with a negative multiplier leave the set,
   violated rows enter it, and the round is repeated, MPCX_POLISH_TRIES times in all; after that nothing is kept and the iteration goes on
   (or ends with its own iterate).  Polish rounds are not counted as iterations. */
#define MPCX_POLISH_MU 1e-5         /* entry: mu, primal residual / hnorm, dual residual / gnorm predicted below these (or any exit) */
#define MPCX_POLISH_RP 1e-6
#define MPCX_POLISH_RD 1e-3
#define MPCX_POLISH_RHO 1e8         /* penalty of the augmented-Lagrangian solve */
#define MPCX_POLISH_TRIES 3
#define MPCX_POLISH_EPS_L 1e-9      /* a new multiplier below -EPS_L / a gap above EPS_G rejects the point */
#define MPCX_POLISH_EPS_G 1e-9
