"""Sampling tables for the denoise loop: Euler-discrete, DPM-Solver++(2M), and the stochastic Euler ancestral and
DPM++ 2M SDE, with optional Karras sigmas.

The reference does not contain a scheduler: its 50-step loop is the
third-party Diffusers SDXL pipeline (diffusers==0.21.2, requirements.txt:1;
call site implementations/Diffusers/load_sdxl_pipeline.py:39-46) driving
`pipe.unet` once per step.  This module restates the published
EulerDiscreteScheduler arithmetic with the SDXL-base scheduler settings
(scaled-linear betas 0.00085..0.012, 1000 train steps, "leading" spacing,
steps_offset 1, epsilon prediction) so the loop can run on-device inside a
hipGraph.  Parity for this arithmetic is not pinned by any reference test
(SURVEY.md 8c-ii): the oracle drives the reference UNet with the same tables.

Karras sigmas (`karras=True`; Karras et al. 2022, eq. 5, rho = 7): n sigmas from the largest to the smallest training
sigma, sigma_i = (sigma_max^(1/rho) + i/(n-1) (sigma_min^(1/rho) - sigma_max^(1/rho)))^rho, then a final 0.  The timestep
of sigma_i is the fractional t in [0, 999] at which log(training sigma), linearly interpolated over the integer t, equals
log(sigma_i) (diffusers' `_sigma_to_t`); it is not rounded.

DPM-Solver++(2M) (Lu et al. 2022, data prediction, multistep; the sigma form of k-diffusion's `sample_dpmpp_2m`).  With
lambda_i = -log sigma_i, h_i = lambda_{i+1} - lambda_i and e the (guided) eps of step i:
    d_i     = x_i - sigma_i e_i                                  the prediction of the clean latent
    a_i     = sigma_{i+1} / sigma_i,   b_i = -expm1(-h_i)        (last step: sigma_{i+1} = 0, a = 0, b = 1, so x = d)
    k_i     = 0 on a first-order step, else 1 / (2 r_i) with r_i = (lambda_i - lambda_{i-1}) / h_i
    x_{i+1} = a_i x_i + b_i ((1 + k_i) d_i - k_i d_{i-1})
A step is first-order when it is the first after the trajectory's start (step 0, or an img2img start) or the last one.
The UNet input is x in_scale, as for Euler.  The loop keeps d_{i-1} in an fp32 history buffer between steps.

Stochastic samplers (SDETables): the DPM++ row plus fresh Gaussian noise z_i on every step, one row form for both,
    x_{i+1} = a_i x_i + b_i ((1 + k_i) d_i - k_i d_{i-1}) + c_i z_i          z_i ~ N(0, 1) per element
with s = sigma_i, s' = sigma_{i+1}, eta (0: no noise) and s_noise (noise multiplier):
  Euler ancestral (k-diffusion's `sample_euler_ancestral`, diffusers' EulerAncestralDiscreteScheduler):
    sigma_up = min(s', eta sqrt(s'^2 (s^2 - s'^2) / s^2)),  sigma_down = sqrt(s'^2 - sigma_up^2)
    a = sigma_down / s,  b = 1 - a,  k = 0,  c = s_noise sigma_up          i.e. x + (sigma_down - s) e + sigma_up z
  DPM++ 2M SDE, midpoint (k-diffusion's `sample_dpmpp_2m_sde`, diffusers' algorithm_type="sde-dpmsolver++"):
    a = (s'/s) exp(-eta h),  b = -expm1(-(1 + eta) h),  k = 1/(2 r) as for DPM++(2M) (0 on a first-order step),
    c = s_noise s' sqrt(-expm1(-2 eta h))
  Last row (s' = 0), both: [s, 0, 1, 0, 0], so x = d and no noise is drawn.
With eta = 0 the DPM++ 2M SDE rows are the DPM++(2M) rows, bit for bit, with c = 0.  The noise z_i is the counter-based
stream of rng.py at counter word i + 1 (i the absolute schedule index), keyed by the sample's seed.

Diffusers versions discretise the timesteps differently: 0.21.2, which the reference pins, rounds t and ends the Karras
schedule at sigma(t=0).  Parity with any diffusers version stays unpinned, as it already is for Euler.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class _SigmaTables:
    timesteps: np.ndarray      # (n,) float32, value fed to the UNet each step
    sigmas: np.ndarray         # (n+1,) float32, last entry 0
    init_noise_sigma: float

    @property
    def n_steps(self) -> int:
        return len(self.timesteps)

    def in_scale(self) -> np.ndarray:
        """1/sqrt(sigma^2+1): latent -> UNet input scaling per step."""
        s = self.sigmas[:-1].astype(np.float64)
        return (1.0 / np.sqrt(s * s + 1.0)).astype(np.float32)


@dataclass(frozen=True)
class EulerTables(_SigmaTables):
    def dsigma(self) -> np.ndarray:
        """sigma[i+1]-sigma[i]: x <- x + eps * dsigma (epsilon prediction)."""
        s = self.sigmas.astype(np.float64)
        return (s[1:] - s[:-1]).astype(np.float32)


@dataclass(frozen=True)
class DPMSolverTables(_SigmaTables):
    def coefficients(self) -> np.ndarray:
        """(n, 4) float32, one row [sigma_i, a_i, b_i, k_i] per step (module docstring), computed in float64 from the
        stored sigmas.  Row 0 and the last row are first-order (k = 0)."""
        s = self.sigmas.astype(np.float64)
        n = self.n_steps
        rows = np.zeros((n, 4), dtype=np.float64)
        lam = -np.log(s[:-1])                       # lambda_0 .. lambda_{n-1}; lambda_n = inf (sigma_n = 0)
        for i in range(n):
            rows[i, 0] = s[i]
            if i == n - 1 or s[i + 1] == 0.0:
                rows[i, 1], rows[i, 2] = 0.0, 1.0
                continue
            h = lam[i + 1] - lam[i]
            rows[i, 1] = s[i + 1] / s[i]
            rows[i, 2] = -np.expm1(-h)
            if i > 0:
                r = (lam[i] - lam[i - 1]) / h
                rows[i, 3] = 1.0 / (2.0 * r)
        return rows.astype(np.float32)


@dataclass(frozen=True)
class SDETables(_SigmaTables):
    """Tables of a stochastic sampler: `sampler` is "euler_ancestral" or "dpmpp_2m_sde" (module docstring)."""
    sampler: str = "dpmpp_2m_sde"
    eta: float = 1.0
    s_noise: float = 1.0

    def __post_init__(self):
        if self.sampler not in ("euler_ancestral", "dpmpp_2m_sde"):
            raise ValueError(f"SDETables: unknown sampler {self.sampler!r} (euler_ancestral or dpmpp_2m_sde)")
        if not self.eta >= 0.0 or not self.s_noise >= 0.0:
            raise ValueError(f"SDETables: eta ({self.eta}) and s_noise ({self.s_noise}) must be >= 0")

    def coefficients(self) -> np.ndarray:
        """(n, 5) float32, one row [sigma_i, a_i, b_i, k_i, c_i] per step (module docstring), computed in float64 from the
        stored sigmas.  The last row is [sigma, 0, 1, 0, 0]."""
        s = self.sigmas.astype(np.float64)
        n = self.n_steps
        eta, s_noise = float(self.eta), float(self.s_noise)
        rows = np.zeros((n, 5), dtype=np.float64)
        lam = -np.log(s[:-1])                       # the expressions of DPMSolverTables.coefficients(): eta = 0 gives its bits
        for i in range(n):
            rows[i, 0] = s[i]
            if i == n - 1 or s[i + 1] == 0.0:
                rows[i, 1], rows[i, 2] = 0.0, 1.0
                continue
            if self.sampler == "euler_ancestral":
                sc, sn = s[i], s[i + 1]
                up = min(sn, eta * np.sqrt(sn * sn * (sc * sc - sn * sn) / (sc * sc)))
                down = np.sqrt(sn * sn - up * up)
                rows[i, 1] = down / sc
                rows[i, 2] = 1.0 - rows[i, 1]
                rows[i, 4] = s_noise * up
                continue
            h = lam[i + 1] - lam[i]
            rows[i, 1] = s[i + 1] / s[i] * np.exp(-eta * h)
            rows[i, 2] = -np.expm1(-(1.0 + eta) * h)
            if i > 0:
                r = (lam[i] - lam[i - 1]) / h
                rows[i, 3] = 1.0 / (2.0 * r)
            rows[i, 4] = s_noise * s[i + 1] * np.sqrt(-np.expm1(-2.0 * eta * h))
        return rows.astype(np.float32)


def training_sigmas(n_train: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012) -> np.ndarray:
    """float64 sigma of every training timestep t = 0 .. n_train - 1 (scaled-linear betas), increasing in t."""
    betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, n_train, dtype=np.float64) ** 2
    alphas_cumprod = np.cumprod(1.0 - betas)
    return np.sqrt((1.0 - alphas_cumprod) / alphas_cumprod)


def sigma_to_t(sigmas: np.ndarray, all_sigmas: np.ndarray) -> np.ndarray:
    """Fractional timestep of each sigma: log(all_sigmas[t]) interpolated linearly over the integer t, inverted (clipped to
    [0, n_train - 1]).  A sigma equal to a training sigma gives its integer t."""
    log_all = np.log(all_sigmas)
    return np.interp(np.log(np.maximum(np.asarray(sigmas, dtype=np.float64), 1e-10)), log_all,
                     np.arange(len(all_sigmas), dtype=np.float64))


def karras_sigmas(n_steps: int, sigma_min: float, sigma_max: float, rho: float = 7.0) -> np.ndarray:
    """float64 (n,) Karras sigmas from sigma_max down to sigma_min (no final 0)."""
    ramp = np.arange(n_steps, dtype=np.float64) / max(n_steps - 1, 1)
    lo, hi = sigma_min ** (1.0 / rho), sigma_max ** (1.0 / rho)
    return (hi + ramp * (lo - hi)) ** rho


def euler_discrete_tables(n_steps: int = 50, n_train: int = 1000, beta_start: float = 0.00085,
                          beta_end: float = 0.012, steps_offset: int = 1, karras: bool = False) -> EulerTables:
    all_sigmas = training_sigmas(n_train, beta_start, beta_end)
    if karras:
        sig = karras_sigmas(n_steps, float(all_sigmas.min()), float(all_sigmas.max()))
        ts = sigma_to_t(sig, all_sigmas)
    else:
        ratio = n_train // n_steps
        ts = (np.arange(0, n_steps) * ratio).round()[::-1].astype(np.float64) + steps_offset
        sig = np.interp(ts, np.arange(n_train, dtype=np.float64), all_sigmas)
    sig = np.concatenate([sig, [0.0]])
    init = float(np.sqrt(sig.max() ** 2 + 1.0))
    return EulerTables(ts.astype(np.float32), sig.astype(np.float32), init)


def dpmpp_2m_tables(n_steps: int = 25, n_train: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                    steps_offset: int = 1, karras: bool = False) -> DPMSolverTables:
    """DPM-Solver++(2M) tables: the timesteps, sigmas and init sigma of `euler_discrete_tables` with the same arguments."""
    e = euler_discrete_tables(n_steps, n_train, beta_start, beta_end, steps_offset, karras)
    return DPMSolverTables(e.timesteps, e.sigmas, e.init_noise_sigma)


def euler_ancestral_tables(n_steps: int = 50, n_train: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                           steps_offset: int = 1, eta: float = 1.0, s_noise: float = 1.0, karras: bool = False) -> SDETables:
    """Euler ancestral ("Euler a") tables: the timesteps, sigmas and init sigma of `euler_discrete_tables` with the same
    arguments."""
    e = euler_discrete_tables(n_steps, n_train, beta_start, beta_end, steps_offset, karras)
    return SDETables(e.timesteps, e.sigmas, e.init_noise_sigma, "euler_ancestral", float(eta), float(s_noise))


def dpmpp_2m_sde_tables(n_steps: int = 25, n_train: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                        steps_offset: int = 1, eta: float = 1.0, s_noise: float = 1.0, karras: bool = False) -> SDETables:
    """DPM++ 2M SDE (midpoint) tables: the timesteps, sigmas and init sigma of `euler_discrete_tables` with the same
    arguments."""
    e = euler_discrete_tables(n_steps, n_train, beta_start, beta_end, steps_offset, karras)
    return SDETables(e.timesteps, e.sigmas, e.init_noise_sigma, "dpmpp_2m_sde", float(eta), float(s_noise))
