// GPU run of the NodeJS host (tests/test_gpu_recommend_resident.py): warm-starts from the factor files Python wrote into
// <dir>/ml_factors_ready, trains, and answers recommendItemsForUsers from the trained handle.
'use strict';
const path = require('path');
const fs = require('fs');
const root = path.join(__dirname, '..', '..', 'you-can-not-recommend_amd');
const Emf = require(path.join(root, 'lib', 'emf', 'Emf'));
const { Dataset } = require(path.join(root, 'lib', 'Dataset'));

const input = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const F = input.useDoublePrecision ? Float64Array : Float32Array;
const t = { user: Int32Array.from(input.user), item: Int32Array.from(input.item), rating: F.from(input.rating) };
const ds = new Dataset(input.users, input.items, t, Int8Array.from(input.type), F);
const lord = Emf.createLord();
lord.init({}, { factorsCount: input.k, trainIters: input.iters, dataDir: input.dir, dbType: 'ml', useDoublePrecision: input.useDoublePrecision,
  ratingsInPortionForRmse: input.rip, numThreadsForTrain: { als: input.threads } });
lord.train(ds).then(() => {
  const recs = lord.recommendItemsForUsers(input.userIds, input.limit, input.minRecommendRating, input.unratedItems);
  // the refusal where the user matrix is not replicated on the rank
  let bandsError = null;
  const bands = lord.bands, world = lord.options.world;
  lord.bands = [0, input.users]; lord.options.world = 2;
  try { lord.recommendItemsForUsers(input.userIds, input.limit); } catch (e) { bandsError = e.message; }
  lord.bands = bands; lord.options.world = world;
  console.log(JSON.stringify({ recs, bandsError }));
  lord.destroy();
}).catch((e) => { console.error(e); process.exit(1); });
