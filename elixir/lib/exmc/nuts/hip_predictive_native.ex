defmodule Exmc.NUTS.HipPredictiveNative do
  @moduledoc """
  NIF binding of `libexmc_hip.so`'s posterior predictive sampling (`include/exmc_hip_predictive.h`,
  DESIGN.md "Posterior predictive"): replicates of every datum of a built model kind, drawn on the device
  with one generator per chain. The C side is `c_src/exmc_hip_predictive_nif.c`, a module beside
  `Exmc.NUTS.HipCompareNative`; conventions are HipNative's. `Exmc.NUTS.HipPredictive.posterior_predictive/3`
  is the caller.

  Load: `priv/exmc_hip_predictive_nif.so` (build line in `INTEGRATION.md`); `EXMC_HIP_DEVICE` selects the GPU.
  """

  @on_load :load_nif

  @doc false
  def load_nif do
    path = :filename.join(:code.priv_dir(:exmc), ~c"exmc_hip_predictive_nif")

    case :erlang.load_nif(path, 0) do
      :ok -> :ok
      {:error, _reason} -> :ok
    end
  end

  @doc """
  model = {kind, data_bin} as `HipNative.model_create/2` takes them; draws: `[chain][draw][dim]` f64
  binary in kernel order, as HipNative's sampling functions return it; chain c draws with
  seed + 7919 (chain_lo + c) -> `[chain][draw][datum]` f64 binary (datums in the kind's data order)
  """
  def posterior_predictive(_model, _draws, _n_chains, _n_draws, _seed, _chain_lo),
    do: :erlang.nif_error(:nif_not_loaded)
end
