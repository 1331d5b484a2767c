// wf_phat.hpp -- the constant of the floored PHAT weighting (include/wf_hip.h, "inter-channel delay": b), shared by the kernels that
// weight a cross spectrum with it: wf_delay.hpp, and wf_xfer_sums.hpp for wf_xfer.hpp and wf_impulse.hpp.
#pragma once

namespace wf {

constexpr double WF_DELAY_BETA = 1e-3; // the floor of the PHAT weighting: 60 dB under the strongest cross-power

} // namespace wf
