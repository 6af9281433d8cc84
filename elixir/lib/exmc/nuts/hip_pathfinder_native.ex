defmodule Exmc.NUTS.HipPathfinderNative do
  @moduledoc """
  NIF binding of `libexmc_hip.so`'s Pathfinder (`include/exmc_hip_pathfinder.h`, DESIGN.md "Pathfinder"):
  `Exmc.Pathfinder` of a built model kind with one L-BFGS path per lane group, all paths of a call in one
  launch. The C side is `c_src/exmc_hip_pathfinder_nif.c`, a module beside `Exmc.NUTS.HipPsisNative`;
  conventions are HipNative's. `Exmc.NUTS.HipPathfinder.fit/2` is the caller.

  Load: `priv/exmc_hip_pathfinder_nif.so` (build line in `INTEGRATION.md`); `EXMC_HIP_DEVICE` selects the GPU.
  """

  @on_load :load_nif

  @doc false
  def load_nif do
    path = :filename.join(:code.priv_dir(:exmc), ~c"exmc_hip_pathfinder_nif")

    case :erlang.load_nif(path, 0) do
      :ok -> :ok
      {:error, _reason} -> :ok
    end
  end

  @doc """
  model = {kind, data_bin} as `HipNative.model_create/2` takes them; perm as `HipNative.model_set_flat_order/2`
  takes it (`[]`: kernel order); path c runs with seed + 7919 (chain_lo + c) ->
  `{draws [path][draw][dim], mu [path][dim], sigma [path][dim], elbo [path]}` as f64 binaries in kernel
  order and unconstrained space, then `{num_iters, best_index, status}` as i32 binaries `[path]`, all in
  one 7-tuple. `lanes` 0 is the kind's default layout.
  """
  def fit(_model, _perm, _n_paths, _chain_lo, _num_draws, _max_iters, _history_size, _seed, _lanes),
    do: :erlang.nif_error(:nif_not_loaded)
end
