defmodule Exmc.NUTS.HipPriorNative do
  @moduledoc """
  NIF binding of `libexmc_hip.so`'s prior sampling (`include/exmc_hip_prior.h`, DESIGN.md "Prior
  predictive"): draws of every free variable of a built model kind from its prior and replicates of every
  datum, drawn on the device with one generator per chain. The C side is `c_src/exmc_hip_prior_nif.c`, a
  module beside `Exmc.NUTS.HipPredictiveNative`; conventions are HipNative's.
  `Exmc.NUTS.HipPrior.prior_samples/3` is the caller.

  Load: `priv/exmc_hip_prior_nif.so` (build line in `INTEGRATION.md`); `EXMC_HIP_DEVICE` selects the GPU.
  """

  @on_load :load_nif

  @doc false
  def load_nif do
    path = :filename.join(:code.priv_dir(:exmc), ~c"exmc_hip_prior_nif")

    case :erlang.load_nif(path, 0) do
      :ok -> :ok
      {:error, _reason} -> :ok
    end
  end

  @doc """
  model = {kind, data_bin} as `HipNative.model_create/2` takes them; chain c draws with
  seed + 7919 (chain_lo + c); replicates is 0 or 1 -> `{x, q, yrep}`: `[chain][draw][dim]` f64 binaries of
  the constrained values and of the unconstrained position (kernel order), and the `[chain][draw][datum]`
  replicates (datums in the kind's data order; an empty binary with replicates = 0)
  """
  def prior_samples(_model, _n_chains, _n_draws, _seed, _chain_lo, _replicates),
    do: :erlang.nif_error(:nif_not_loaded)
end
